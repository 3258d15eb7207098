"""GPU: the decode path (what generate() runs) against plain fp64 references.

  * dg_attn_decode / dg_attn_decode_append against oracle.parity.decode_attention_fp64 at the head sizes, key counts and LDS
    requests the model tests never reach, bit for bit against the generic forward's row t, inside guard bands and over
    NaN-poisoned cache rows; dg_embed_window at odd widths and past its workgroup cap;
  * dg_gemm_nt at M = B = 1 .. 3 rows with the four epilogues of a decode step, the plain one into a row of the K/V cache
    (ldc = Tcap * N);
  * TransformerLM at H = 64, ctx = 130, B = 3: every cached position against the CPU oracle, the bf16 hand-over from the MFMA
    prefill to the generic decode kernel, token equality across the window slide, and a DeviceDecoder that is used again.

Bounds are the project's own (tests/test_gpu_ops.py, tests/test_gpu_bf16x3.py, tests/test_gpu_models.py) or derived in
oracle/parity.py; the values the kernels reach on the MI355X stand beside the cases.  DG_TEST_REPORT=1 prints them."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

f32, bf = torch.float32, torch.bfloat16
GUARD = 256
FILL = 55.0                     # exactly representable in bf16
NAN = float("nan")


def _report(msg):
    if os.environ.get("DG_TEST_REPORT"):
        print("[decode] " + msg, flush=True)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def guarded(shape, dtype, dev, fill=FILL):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fill=FILL):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def bits(x):
    """the bit patterns (NaN rows compare as what they hold)"""
    return x.view(torch.int32 if x.dtype == f32 else torch.int16)


def lds_limit(dev):
    props = torch.cuda.get_device_properties(dev)
    return max(props.shared_memory_per_block, getattr(props, "shared_memory_per_block_optin", 0) or 0)


def raw_attn_decode(cache, out, B, Tcap, t, NH, H):
    """dg_attn_decode's return code, with the caller's (guarded) output"""
    from drakegpt_amd import ops
    from drakegpt_amd._lib import lib
    return lib.dg_attn_decode(cache.data_ptr(), out.data_ptr(), B, Tcap, t, NH, H, float(H ** -0.5), ops.dt_code(cache.dtype),
                              torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the two decode-attention kernels against fp64
# ---------------------------------------------------------------------------------------------------------------------
# B, NH, H, Tcap, positions t.  What each row is for:
#   (3, 3, 8, 70)      the lane rounds' edges (t = 63 | 64), a partial second round, B * NH = 9: the last workgroup has one wave
#   (3, 3, 96, 131)    H > 64 and no multiple of 64 (the lane-stride loops over d), a third round of keys
#   (2, 12, 64, 1024)  GPT-2's own geometry; t = 510 (odd t + 1) is where bf16 at H = 64 takes the generic forward
#   (1, 2, 256, 4096)  LDS request 69 632 bytes, above 64 KB
#   (1, 2, 256, 8192)  the entry point's stated limit, 135 168 bytes
#   (1, 1, 128, 200)   one live wave in the only workgroup
# measured on MI355X, worst (b, head) group against fp64 over positions, inputs (randn and the spotlights) and both kernels
# -- which agree to every digit shown --; bounds 2e-5 (fp32) and 3.93e-3 (bf16):
#   shape               fp32      bf16
#   (3, 3, 8, 70)       3.8e-7    3.2e-3
#   (3, 3, 96, 131)     9.6e-7    2.0e-3
#   (2, 12, 64, 1024)   1.3e-6    2.2e-3
#   (1, 2, 256, 4096)   2.0e-6    1.7e-3
#   (1, 2, 256, 8192)   2.6e-6    1.8e-3
#   (1, 1, 128, 200)    8.3e-7    1.9e-3
# and every position that has a generic forward to compare with is bit-identical to it, in both dtypes.
DECODE_SHAPES = [
    (3, 3, 8, 70, (0, 1, 63, 64, 69)),
    (3, 3, 96, 131, (64, 127, 128, 130)),
    (2, 12, 64, 1024, (510, 511, 1023)),
    (1, 2, 256, 4096, (4095,)),
    (1, 2, 256, 8192, (8191,)),
    (1, 1, 128, 200, (199,)),
]


def _generic_forward(dtype, H, T):
    """does ops.attn_fwd take the generic fp32-arithmetic kernels at this shape?  (bf16 at H = 64 with even T: the MFMA kernels)"""
    return T <= 4096 and not (dtype == bf and H == 64 and T % 2 == 0)


def _decode_inputs(kind, B, Tcap, NH, H, t, seed, dtype):
    from oracle import parity as P
    if kind == "randn":
        host = torch.randn((B, Tcap, 3 * NH * H), generator=torch.Generator().manual_seed(seed)).to(dtype)
    else:
        host = P.spotlight_decode_inputs(B, Tcap, NH, H, t, kind, seed, dtype)
    host[:, t + 1:] = NAN                                        # nothing past t may be read
    return host


def _decode_position(dev, dtype, B, NH, H, Tcap, t, kind, seed):
    from drakegpt_amd import ops
    from oracle import parity as P
    W = 3 * NH * H
    name = f"decode {'bf16' if dtype == bf else 'fp32'} {(B, NH, H, Tcap)} t={t} {kind}"
    host = _decode_inputs(kind, B, Tcap, NH, H, t, seed, dtype)
    ref, _ = P.decode_attention_fp64(host, t, B, Tcap, NH, H)
    want = host.to(dev)
    # dg_attn_decode: the cache is read only
    cbuf, cache = guarded((B, Tcap, W), dtype, dev)
    cache.copy_(want)
    obuf, out = guarded((B, NH * H), dtype, dev)
    assert raw_attn_decode(cache, out, B, Tcap, t, NH, H) == 0
    torch.cuda.synchronize()
    assert guards_intact(cbuf) and guards_intact(obuf), name
    assert torch.equal(bits(cache), bits(want)), name
    e1 = P.assert_decode_output(out, ref, H, dtype, name)
    # dg_attn_decode_append: row t arrives in the staging row; the cache holds something else there
    row = want[:, t].contiguous()
    cbuf2, cache2 = guarded((B, Tcap, W), dtype, dev)
    cache2.copy_(want)
    cache2[:, t] = torch.randn((B, W), generator=torch.Generator().manual_seed(seed + 1)).to(dtype).to(dev)
    obuf2, out2 = guarded((B, NH * H), dtype, dev)
    ops.attn_decode_append(row, cache2, ops.new_rng_state(0, dev, step=t + 1), NH, H, H ** -0.5, out=out2)
    torch.cuda.synchronize()
    assert guards_intact(cbuf2) and guards_intact(obuf2), name
    assert torch.equal(bits(cache2), bits(want)), name           # row t == row, every other byte as it was
    e2 = P.assert_decode_output(out2, ref, H, dtype, name + " (append)")
    # the documented contract: the arithmetic and its order are those of the generic forward for query row t
    exact = None
    if _generic_forward(dtype, H, t + 1) and (t < 1024 or kind in ("randn", t)):
        full, _ = ops.attn_fwd(want[:, :t + 1].reshape(B * (t + 1), W).contiguous(), B, t + 1, NH, H, H ** -0.5, 0.0, None, 0)
        last = full.view(B, t + 1, NH * H)[:, t]
        exact = (torch.equal(out, last), torch.equal(out2, last))
        assert all(exact), (name, "not bit-identical to attn_fwd's row t (decode, append):", exact,
                            (out.float() - last.float()).abs().max().item(), (out2.float() - last.float()).abs().max().item())
    return max(e1, e2), exact is not None


@pytest.mark.parametrize("dtype", [f32, bf], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,NH,H,Tcap,ts", DECODE_SHAPES)
def test_attn_decode_against_fp64(dev, dtype, B, NH, H, Tcap, ts):
    lds = 4 * (Tcap + H) * 4                                     # AS_WAVES * (Tcap + H) floats
    if lds > 65536:                                              # read from the host, not found out by launching
        assert (Tcap, H, lds) in ((4096, 256, 69632), (8192, 256, 135168))
        assert lds <= lds_limit(dev), (lds, lds_limit(dev))
    worst, n_exact = 0.0, 0
    for t in ts:
        kinds = ["randn"] + (sorted({t, 0, 64 * (t // 64), t - 1}) if t >= 1 else [])
        for i, kind in enumerate(kinds):
            e, exact = _decode_position(dev, dtype, B, NH, H, Tcap, t, kind, 1000 * H + 10 * t + i)
            worst, n_exact = max(worst, e), n_exact + exact
    _report(f"attention {'bf16' if dtype == bf else 'fp32'} {(B, NH, H, Tcap)}: worst group {worst:.2e}; "
            f"{n_exact} inputs bit-identical to the generic forward")
    # every shape but the 8192-key one (fp32) and GPT-2's even lengths (bf16) has positions on the generic forward
    assert (n_exact > 0) == any(_generic_forward(dtype, H, t + 1) for t in ts)


def test_attn_decode_rejections_leave_the_buffers_untouched(dev):
    """every refusal is a return code or a Python check in front of the launch: nothing runs, nothing is written"""
    from drakegpt_amd import ops
    B, NH, H, Tcap = 2, 2, 8, 16
    s = H ** -0.5
    bufs = []

    def g(shape, dtype=f32):
        buf, view = guarded(shape, dtype, dev)
        bufs.append(buf)
        return view

    cache, out, row = g((B, Tcap, 3 * NH * H)), g((B, NH * H)), g((B, 3 * NH * H))
    st = ops.new_rng_state(0, dev, step=3)
    assert raw_attn_decode(cache, out, B, Tcap, 2, NH, H) == 0           # (the accepted call, so that the refusals mean something)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    out.fill_(FILL)
    for t in (Tcap, Tcap + 7, -1):
        assert raw_attn_decode(cache, out, B, Tcap, t, NH, H) == -1      # DG_ERR_ARG
        with pytest.raises(RuntimeError, match="dg_attn_decode failed"):
            ops.attn_decode(cache, t, NH, H, s)
    # H = 257 and Tcap = 8193: one past what the entry points state
    c257, o257, r257 = g((1, 2, 3 * 257)), g((1, 257)), g((1, 3 * 257))
    assert raw_attn_decode(c257, o257, 1, 2, 1, 1, 257) == -1
    with pytest.raises(RuntimeError, match="dg_attn_decode failed"):
        ops.attn_decode(c257, 1, 1, 257, s)
    with pytest.raises(RuntimeError, match="dg_attn_decode_append failed"):
        ops.attn_decode_append(r257, c257, st, 1, 257, s, out=o257)
    c8193, o8, r8 = g((1, 8193, 3 * 8)), g((1, 8)), g((1, 3 * 8))
    assert raw_attn_decode(c8193, o8, 1, 8193, 0, 1, 8) == -1
    with pytest.raises(RuntimeError, match="dg_attn_decode failed"):
        ops.attn_decode(c8193, 0, 1, 8, s)
    with pytest.raises(RuntimeError, match="dg_attn_decode_append failed"):
        ops.attn_decode_append(r8, c8193, st, 1, 8, s, out=o8)
    # a cache width that is not 3 * NH * H
    with pytest.raises(RuntimeError, match="width"):
        ops.attn_decode(cache, 2, NH, H + 1, s)
    with pytest.raises(RuntimeError, match="cache must be"):
        ops.attn_decode_append(row, cache, st, NH + 1, H, s, out=out)
    with pytest.raises(RuntimeError, match="cache must be"):
        ops.attn_decode_append(g((B, 3 * NH * H + 1)), cache, st, NH, H, s, out=out)
    # row and cache of different dtypes; an output of the wrong shape or dtype
    with pytest.raises(TypeError):
        ops.attn_decode_append(g((B, 3 * NH * H), bf), cache, st, NH, H, s, out=out)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.attn_decode_append(row, cache, st, NH, H, s, out=g((B, NH * H + 1)))
    with pytest.raises(RuntimeError, match="out must be"):
        ops.attn_decode_append(row, cache, st, NH, H, s, out=g((B + 1, NH * H)))
    with pytest.raises(TypeError):
        ops.attn_decode_append(row, cache, st, NH, H, s, out=g((B, NH * H), bf))
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf == FILL).all())


def test_embed_window_odd_widths_and_grid_stride(dev):
    """what test_embed_window_equals_embed_fwd leaves out: C = 7 (odd, part of one lane round), C = 200 (four rounds, the last
    partial), and mode 1 with 5 * 4096 rows -- more waves than the capped grid of 4096 workgroups has, so the loop strides"""
    from drakegpt_amd import ops
    V = 80
    for C, B, Tw, cap in ((7, 3, 65, 90), (200, 3, 65, 90), (8, 5, 4096, 4100)):
        g = torch.Generator().manual_seed(C)
        ids = torch.randint(0, V, (B, cap), generator=g).to(dev)
        ids[0, 3], ids[B - 1, cap - 2] = V + 5, -2                 # clamped like dg_embed_fwd clamps
        tok, pos = torch.randn((V, C), generator=g).to(dev), torch.randn((Tw, C), generator=g).to(dev)
        for t in (0, 3, 64):                                       # mode 0 at position t = L - 1
            buf, out = guarded((B, C), f32, dev)
            ops.embed_window(ids, ops.new_rng_state(0, dev, step=t + 1), tok, pos, 0, out=out)
            ref = ops.embed_fwd(ids[:, t:t + 1].contiguous(), tok, pos[t:t + 1])
            assert torch.equal(out, ref.view(B, C)) and guards_intact(buf), (C, t)
        for L in (Tw, cap - 1, cap):                               # mode 1: the last Tw ids
            buf, out = guarded((B, Tw, C), f32, dev)
            ops.embed_window(ids, ops.new_rng_state(0, dev, step=L), tok, pos, 1, out=out)
            ref = ops.embed_fwd(ids[:, L - Tw:L].contiguous(), tok, pos)
            assert torch.equal(out, ref) and guards_intact(buf), (C, L)


# ---------------------------------------------------------------------------------------------------------------------
# 4. dg_gemm_nt at M = B rows
# ---------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [
    (192, 64),          # generic kernel, K < 128
    (2304, 768),        # 128 x 192 tiles, GPT-2's QKV
    (768, 3072),
    (3072, 768),
    (80, 128),          # ragged N
    (50257, 768),       # lm_head: odd ldc, scalar stores
]
GEMM_TCAP, GEMM_T = 16, 5      # the plain epilogue writes row 5 of a [M, 16, N] cache: ldc = 16 * N
# Tolerances, whole tensor and per output row alike (the existing tests of the same form): fp32 operands 2e-6 plain and 1e-5
# with an epilogue; split 1e-5; bf16 OUTPUT 6e-3 and every element within one bf16 rounding of fp64 plus the fp32
# accumulation envelope.  bf16 operands with an fp32 output: the products of bf16 operands are exact in fp32 and the
# reference takes the same rounded operands, so what is left is the fp32 accumulation -- the fp32 figures hold (the decode
# step's plain GEMM writes bf16; the fp32-output plain form of test_gemm_nt_plain is launched as well, at its 2e-6).
# measured on MI355X, worst output row over M = 1 .. 3 and the epilogues:
#   fp32 operands        1.5e-7 (K = 64) .. 1.1e-6 (K = 3072), the same for every epilogue
#   bf16, bf16 output    1.6e-3 .. 1.9e-3 (plain and bias + ReLU); fp32 output 4.3e-8 .. 3.5e-7
#   split                4.4e-6 .. 5.3e-6


def _mm64(A, Bm, chunk=8192):
    """A @ Bm^T in fp64 without an fp64 copy of the whole of Bm (154 MB lm_head)"""
    return torch.cat([A.double() @ Bm[i:i + chunk].double().T for i in range(0, Bm.shape[0], chunk)], 1)


def _envelope(A, Bm, K, bias=None, chunk=8192):
    from oracle import parity as P
    return torch.cat([P.gemm_envelope(A, Bm[i:i + chunk], K, None if bias is None else bias[i:i + chunk])
                      for i in range(0, Bm.shape[0], chunk)], 1)


@pytest.mark.parametrize("form", ["fp32", "bf16", "split"])
@pytest.mark.parametrize("N,K", GEMM_SHAPES)
def test_gemm_nt_decode_rows(dev, N, K, form):
    from drakegpt_amd import ops
    from oracle import parity as P
    dt, split = (bf if form == "bf16" else f32), form == "split"
    g = torch.Generator().manual_seed(N + K)
    A3, Bm = torch.randn(3, K, generator=g).to(dt), torch.randn(N, K, generator=g).to(dt)
    bias, resid3 = torch.randn(N, generator=g), torch.randn(3, N, generator=g)
    acc3 = _mm64(A3, Bm)
    Abuf = torch.full((128, K), NAN, dtype=dt, device=dev)                 # the rest of a 128-row tile is poison
    Abuf[:3] = A3.to(dev)
    Bd, bd, rd = Bm.to(dev), bias.to(dev), resid3.to(dev)
    tol_plain = 1e-5 if split else (6e-3 if dt == bf else 2e-6)
    tol_f32out = 1e-5
    tol_act = 6e-3 if dt == bf else 1e-5
    env3 = _envelope(A3, Bm, K) if dt == bf else None
    envb3 = _envelope(A3, Bm, K, bias) if dt == bf else None
    worst = {}

    def check(got, ref, tol, what, M):
        assert rel(got, ref) < tol, (what, M, rel(got, ref))
        worst[what] = max(worst.get(what, 0.0), P.assert_rowwise(got, ref, N, tol, f"gemm {form} {N}x{K} M={M} {what}"))

    for M in (1, 2, 3):
        A, acc = Abuf[:M], acc3[:M]
        # plain, into row GEMM_T of a NaN-filled [M, Tcap, N] cache inside guard bands
        buf, body = guarded((M, GEMM_TCAP, N), dt, dev, NAN)
        snap = bits(buf).clone()
        out = body[:, GEMM_T]
        assert out.stride(0) == GEMM_TCAP * N
        ops.gemm_nt(A, Bd, dt, out=out, split=split)
        torch.cuda.synchronize()
        got = out.clone()
        body[:, GEMM_T] = NAN
        assert torch.equal(bits(buf), snap), (M, "bytes outside row t of the cache changed")
        check(got, acc, tol_plain, "plain", M)
        if dt == bf:
            P.assert_within_rounding(got, acc, env3[:M], 1, f"gemm bf16 {N}x{K} M={M} plain")
            check(ops.gemm_nt(A, Bd, f32), acc, 2e-6, "plain fp32 out", M)
        # bias + residual, fp32 output (proj, second FFN Linear)
        out = ops.gemm_nt(A, Bd, f32, bias=bd, residual=rd[:M], split=split)
        check(out, acc + bias.double() + resid3[:M].double(), tol_f32out, "bias + residual", M)
        # bias + ReLU, activation-dtype output (first FFN Linear)
        out = ops.gemm_nt(A, Bd, dt, bias=bd, relu=True, split=split)
        pre = acc + bias.double()
        check(out, pre.clamp_min(0), tol_act, "bias + relu", M)
        if dt == bf:
            # the share of pre-activations whose sign the envelope leaves open is a property of the operands: the envelope is
            # K * 2^-24 * sum |a||b| ~ 0.64 K^2 * 2^-24 against a pre-activation of deviation sqrt(K), i.e. a share of
            # ~0.5 K^1.5 * 2^-24 (5e-3 at K = 3072); four times that, and two elements of a tensor this small
            decided = P.mask_margin(pre, envb3[:M], max_share=max(1e-3, 2 * K ** 1.5 * 2.0 ** -24 + 2.0 / (M * N)))
            P.assert_within_rounding(out, pre.clamp_min(0), envb3[:M], 1, f"gemm bf16 {N}x{K} M={M} bias + relu", where=decided)
        # bias only, fp32 output (lm_head)
        out = ops.gemm_nt(A, Bd, f32, bias=bd, split=split)
        check(out, pre, tol_f32out, "bias", M)
    _report(f"gemm {form} {N}x{K}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("N,K", [(80, 128), (192, 64), (2304, 768)])
def test_gemm_nt_one_hot_row(dev, N, K):
    """A = e_0 (M = 1) against an asymmetric B: the output is B's column 0, exactly -- the M = 1 counterpart of
    test_gemm_nt_asymmetric_identity.  B holds small integers (exact in bf16, so the split form's lo halves are zero)."""
    from drakegpt_amd import ops
    Bm = ((torch.arange(N * K) * 7) % 253 - 126).float().reshape(N, K)
    assert not torch.equal(Bm[:, 0], Bm[:, 1]) and Bm[:, 0].unique().numel() > 16
    for form in ("fp32", "bf16", "split"):
        dt = bf if form == "bf16" else f32
        Abuf = torch.full((128, K), NAN, dtype=dt, device=dev)
        Abuf[0] = 0
        Abuf[0, 0] = 1
        out = ops.gemm_nt(Abuf[:1], Bm.to(dt).to(dev), f32, split=form == "split")
        assert torch.equal(out.cpu(), Bm[:, 0].view(1, N)), form


# ---------------------------------------------------------------------------------------------------------------------
# 5. the model at H = 64
# ---------------------------------------------------------------------------------------------------------------------
V, C, CTX, NHEADS, LAYERS, BATCH = 80, 128, 130, 2, 2, 3
# whole-tensor bounds of the project: against the fp32 oracle, and (bf16) against the oracle with the kernels' bf16 roundings
WHOLE = {"fp32": (1e-4, None), "bf16x3": (2e-5, None), "bf16": (3e-2, 6e-3)}
# measured on MI355X, worst position (rowwise_rel over V) cached / uncached, and the whole tensor:
#   fp32                          3.5e-7 / 3.5e-7, whole 2.4e-7
#   bf16x3                        6.9e-6 / 6.9e-6, whole 4.8e-6
#   bf16, fp32 oracle             3.4e-3 / 3.4e-3, whole 2.5e-3;  prefill 64 + decode 3.4e-3, whole 2.5e-3
#   bf16, bf16-rounding oracle    2.7e-3 / 3.0e-3, whole 1.2e-3;  prefill 64 + decode 2.2e-3, whole 1.1e-3
_RUNS = {}


def lm(dev, precision="fp32", seed=0):
    import drakegpt_amd as D
    torch.manual_seed(seed)
    return D.TransformerLM(V, C, CTX, NHEADS, LAYERS, 0.1, precision=precision).to(dev).eval()


def nan_caches(m, dev):
    return [torch.full((BATCH, CTX, 3 * C), NAN, dtype=m.act_dtype, device=dev) for _ in m.blocks]


@torch.no_grad()
def run(dev, precision):
    """computed once per precision: the model, a random sequence, the logits of _decode_step at all 130 positions (over
    NaN-filled caches), of the uncached eval forward, and of the CPU oracle on the same state dict"""
    if precision not in _RUNS:
        from oracle import drake_ref as R
        m = lm(dev, precision)
        seq = torch.randint(0, V, (BATCH, CTX), generator=torch.Generator().manual_seed(7)).to(dev)
        ws, w_lm = m._decode_weights()
        caches = nan_caches(m, dev)
        cached = torch.stack([m._decode_step(seq[:, t:t + 1].contiguous(), t, caches, ws, w_lm).clone() for t in range(CTX)], 1)
        full = m(seq)[0]
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        ora = [R.lm_forward("TransformerLM", sd, seq.cpu())[0]]
        if precision == "bf16":
            ora.append(R.lm_forward("TransformerLM", sd, seq.cpu(), bf16=True)[0])
        assert all(torch.isfinite(c).all() for c in caches)               # every row was written before it was read
        _RUNS[precision] = dict(m=m, seq=seq, cached=cached, full=full, ora=ora, ws=ws, w_lm=w_lm)
    return _RUNS[precision]


def _per_position(got, r, precision, what, first=0):
    """whole tensor at the project's bound; per position at most 2 x the worst row of the uncached forward against the same
    oracle (the cached path has the same rounding points, except that its attention keeps P in fp32: no worse), floored at
    the whole-tensor bound"""
    from oracle import parity as P
    for ora, whole in zip(r["ora"], WHOLE[precision]):
        ref = ora[:, first:]
        assert got.shape == ref.shape and torch.isfinite(got).all()
        assert rel(got, ref) < whole, (what, rel(got, ref))
        e_full = P.rowwise_rel(r["full"], ora, V).max().item()
        e_got = P.rowwise_rel(got, ref, V)
        bound = max(2 * e_full, whole)
        _report(f"model {precision} {what}: worst position {e_got.max().item():.2e} (uncached forward {e_full:.2e}), "
                f"whole tensor {rel(got, ref):.2e}, bounds {bound:.2e} / {whole:.0e}")
        assert e_got.max().item() <= bound, (what, int(e_got.argmax()) % ref.shape[1], e_got.max().item(), bound)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x3"])
def test_decode_step_at_every_position_against_the_oracle(dev, precision):
    r = run(dev, precision)
    assert r["cached"].shape == (BATCH, CTX, V)
    _per_position(r["cached"], r, precision, "decode steps")


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_decode_step_is_bit_identical_to_the_uncached_forward(dev, precision):
    """three rounds of keys, H = 64, B * NH = 6 (a partial last workgroup), GEMMs at M = 3 against M = 3 * (t + 1)"""
    r = run(dev, precision)
    with torch.no_grad():
        for t in (63, 64, 127, 128, 129):
            full = r["m"](r["seq"][:, :t + 1].contiguous())[0][:, -1]
            assert torch.equal(r["cached"][:, t], full), (t, (r["cached"][:, t] - full).abs().max().item())


@torch.no_grad()
def test_bf16_prefill_on_the_mfma_kernel_then_decode(dev):
    """64 prompt tokens in one pass (bf16, H = 64, even T: the MFMA attention), the other 66 positions by the generic decode
    kernel on the cache the prefill left"""
    r = run(dev, "bf16")
    m, seq = r["m"], r["seq"]
    caches = nan_caches(m, dev)
    rows = [m._prefill(seq[:, :64].contiguous(), caches, r["ws"], r["w_lm"]).clone()]
    rows += [m._decode_step(seq[:, t:t + 1].contiguous(), t, caches, r["ws"], r["w_lm"]).clone() for t in range(64, CTX)]
    _per_position(torch.stack(rows, 1), r, "bf16", "prefill 64 + decode", first=63)


@torch.no_grad()
def loop(m, idx, n, seed):
    """the reference algorithm with the device sampler (tests/test_gpu_generate_device.py): full forward per token"""
    from drakegpt_amd import ops
    for _ in range(n):
        L = idx.shape[1]
        logits = m(idx[:, -CTX:].contiguous())[0][:, -1]
        idx = torch.cat((idx, ops.sample_rows(logits, seed=seed, L=L)[:, None]), dim=1)
    return idx


def test_generate_tokens_across_64_128_and_the_window_slide(dev):
    m = run(dev, "fp32")["m"]
    prompt = torch.randint(0, V, (BATCH, 5), generator=torch.Generator().manual_seed(2)).to(dev)
    torch.manual_seed(11)
    a = m.generate(prompt, 140, use_cache=False)
    torch.manual_seed(11)
    b = m.generate(prompt, 140, use_cache=True)
    assert a.shape == (BATCH, 145) and torch.equal(a, b)
    d = m.generate(prompt, 140, sampler="device", seed=13)
    assert d.tolist() == loop(m, prompt, 140, 13).tolist()
    assert d.tolist() != m.generate(prompt, 140, sampler="device", seed=14).tolist()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_device_decoder_never_reads_stale_rows(dev, precision):
    """the K/V caches and the staging row of a DeviceDecoder outlive a generate() call: a second, shorter call must read only
    what it wrote itself -- shown with NaN in every row the first call left, then with the first call's own values after a
    run that slid the window"""
    m, fresh = lm(dev, precision), lm(dev, precision)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), fresh.state_dict().values()))
    long = torch.randint(0, V, (BATCH, 9), generator=torch.Generator().manual_seed(3)).to(dev)
    short = long[:, :4].contiguous()
    want = fresh.generate(short, 100, sampler="device", seed=5)
    assert want.shape == (BATCH, 104)
    m.generate(long, 60, sampler="device", seed=5)
    (dec,) = m._decoders.values()
    for t in dec.caches + [dec.row]:
        t.fill_(NAN)
    got = m.generate(short, 100, sampler="device", seed=5)
    assert tuple(m._decoders.values()) == (dec,)                          # the same decoder, the same captured graphs
    assert got.tolist() == want.tolist()
    assert all(torch.isfinite(c[:, :103]).all() and torch.isnan(c[:, 103:]).all() for c in dec.caches)
    m.generate(long, 140, sampler="device", seed=6)                       # 149 tokens: ends in the sliding phase
    assert m.generate(short, 100, sampler="device", seed=5).tolist() == want.tolist()
    assert tuple(m._decoders.values()) == (dec,)
