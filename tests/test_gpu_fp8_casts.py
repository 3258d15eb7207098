"""csrc/fp8.hip on the GPU, branch by branch (tests/fp8_cases.py has the case tables, the host model and the comparison;
tests/test_fp8_cases_host.py accepts them on the CPU): dg_fp8_amax, dg_fp8_quantize and dg_fp8_quantize_delayed through
ops.lib on views between guard bands, byte for byte against the model -- output view, both guard bands, the source, every
partial maximum, the history slots -- with scale_inv held to 1 ulp of the model's fp32 reciprocal; every launch first asserts
that the library's plan for the real addresses of its tensors is the plan the case is named for.  Then every finite bf16
pattern and the rounding boundaries of either format, the non-finite patterns, and an amax below FMAX / FLT_MAX (where
FMAX / amax is +Inf in fp32) for the two entries of fp8.hip and the four other producers that share dg_fp8_scale_of."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_cases as F  # noqa: E402

pytestmark = pytest.mark.gpu

TFMT = {F.E4M3: torch.float8_e4m3fn, F.E5M2: torch.float8_e5m2}
P = F.AMAX_PARTS
GUARD = 777.0                       # around scale_inv and behind the partial maxima
TINY_HISTORY = 2.0 ** -125          # below FMAX / FLT_MAX for both formats


def _report(what, exact):
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[parity] fp8 casts, {what}: scale_inv {'equals' if exact else 'is 1 ulp from'} the fp32 reciprocal", flush=True)


def _np(t):
    return t.detach().cpu().numpy().copy()


def _dt(x):
    return F.BF16 if x.dtype == torch.bfloat16 else F.F32


def _is_the_case(real, named):
    """the library's plan for the tensors actually passed (their real addresses) is the plan the case was named from -- the one
    tests/test_fp8_cases_host.py holds to the case's expectations and the model's partial maxima are computed with"""
    assert real == named, (real, named)


def _amax_launch(ops, dev, x, table=None):
    """dg_fp8_amax on x (flat CPU tensor) between guard bands -> (source bytes, partials [n_seg * P], the P words behind them)"""
    xb = F.source_buffer(x).to(dev)
    ns = len(table) if table else 1
    parts = torch.full(((ns + 1) * P,), GUARD, device=dev)
    seg = torch.tensor(table, dtype=torch.int64, device=dev) if table else None
    assert xb.view.data_ptr() % 16 == 0 and xb.view.numel() == x.numel()
    _is_the_case(F.amax_geometry(_dt(x), x.numel(), table, x_addr=xb.view.data_ptr()), F.amax_geometry(_dt(x), x.numel(), table))
    ops.check(ops.lib.dg_fp8_amax(ops._p(xb.view), ops.dt_code(x.dtype), x.numel(), ops._p(seg), ns, ops._p(parts), ops._stream()), "dg_fp8_amax")
    torch.cuda.synchronize()
    parts = _np(parts)
    return xb.bytes(), parts[:ns * P], parts[ns * P:]


def _quantize_launch(ops, dev, x, fmt, q_off=0, table=None):
    """dg_fp8_amax + dg_fp8_quantize -> the ``got`` of F.compare"""
    n = x.numel()
    xb, qb = F.source_buffer(x).to(dev), F.output_buffer(n, q_off).to(dev)
    ns = len(table) if table else 1
    parts = torch.full(((ns + 1) * P,), GUARD, device=dev)
    sinv = torch.full((ns + 2,), GUARD, device=dev)
    seg = torch.tensor(table, dtype=torch.int64, device=dev) if table else None
    assert xb.view.data_ptr() % 16 == 0 and qb.view.data_ptr() % 16 == q_off and qb.view.numel() == n
    if table:
        assert all(f % 8 == 0 and l % 8 == 0 and 0 <= f and f + l <= n for f, l in table)
    _is_the_case(F.quantize_geometry(_dt(x), n, table, x_addr=xb.view.data_ptr(), q_addr=qb.view.data_ptr()), F.quantize_geometry(_dt(x), n, table, 0, q_off))
    ops.check(ops.lib.dg_fp8_amax(ops._p(xb.view), ops.dt_code(x.dtype), n, ops._p(seg), ns, ops._p(parts), ops._stream()), "dg_fp8_amax")
    ops.check(ops.lib.dg_fp8_quantize(ops._p(xb.view), ops.dt_code(x.dtype), ops._p(qb.view), ops.dt_code(TFMT[fmt]), n, ops._p(seg), ns,
                                      ops._p(parts), ops._p(sinv[1:]), ops._stream()), "dg_fp8_quantize")
    torch.cuda.synchronize()
    parts, sinv = _np(parts), _np(sinv)
    assert np.all(parts[ns * P:] == GUARD) and sinv[0] == GUARD and sinv[-1] == GUARD
    return dict(q=qb.bytes(), x=xb.bytes(), scale_inv=sinv[1:-1], parts=parts[:ns * P])


def _delayed_launch(ops, dev, x, fmt, q_off, prev, step, state=None, parts2=None):
    """dg_fp8_quantize_delayed with the read slot seeded with ``prev`` and the slot to be written holding STALE"""
    n = x.numel()
    xb, qb = F.source_buffer(x).to(dev), F.output_buffer(n, q_off).to(dev)
    parity = step & 1
    if parts2 is None:
        parts2 = torch.full((2 * P,), F.STALE, device=dev)
        parts2[(parity ^ 1) * P:(parity ^ 1) * P + P] = torch.from_numpy(np.asarray(prev, dtype=np.float32)).to(dev)
    if state is None:
        state = ops.new_rng_state(1, dev, step)
    sinv = torch.full((3,), GUARD, device=dev)
    assert xb.view.data_ptr() % 16 == 0 and qb.view.data_ptr() % 16 == q_off and qb.view.numel() == n and parts2.numel() == 2 * P
    _is_the_case(F.delayed_geometry(_dt(x), n, x_addr=xb.view.data_ptr(), q_addr=qb.view.data_ptr()), F.delayed_geometry(_dt(x), n, 0, q_off))
    ops.check(ops.lib.dg_fp8_quantize_delayed(ops._p(xb.view), ops.dt_code(x.dtype), ops._p(qb.view), ops.dt_code(TFMT[fmt]), n, ops._p(parts2),
                                              ops._p(state), ops._p(sinv[1:]), ops._stream()), "dg_fp8_quantize_delayed")
    torch.cuda.synchronize()
    p2, sinv = _np(parts2), _np(sinv)
    assert sinv[0] == GUARD and sinv[2] == GUARD
    return dict(q=qb.bytes(), x=xb.bytes(), scale_inv=sinv[1:2], written=p2[parity * P:parity * P + P],
                read=p2[(parity ^ 1) * P:(parity ^ 1) * P + P]), parts2


# --------------------------------------------------------------------------------------------------------------------- the case tables
@pytest.mark.parametrize("case", F.quantize_cases(), ids=lambda c: c.name)
def test_quantize(dev, case):
    from drakegpt_amd import ops
    if case.seg is None:
        x, _ = F.planted_source(case.dtype, case.n, case.n % 1000 + 3, amp=0.37)
        table = None
    else:
        x, table, _ = F.seg_source(case.dtype, reverse=case.seg)
    want = F.expect_quantize(x, case.fmt, case.q_off, table)
    geo = F.geometry_of(case)
    if case.expect:
        s0, e = geo.segs[0], case.expect
        assert (s0.wide, s0.why, s0.trips, geo.grid) == (e["wide"], e["why"], e["trips"], e["grid"]), (case.name, geo)
    got = _quantize_launch(ops, dev, x, case.fmt, case.q_off, table)
    _report(f"dg_fp8_quantize {case.name}", F.compare(got, want, case.fmt, case.name))


@pytest.mark.parametrize("case", F.delayed_cases(), ids=lambda c: c.name)
def test_quantize_delayed(dev, case):
    from drakegpt_amd import ops
    x, amax = F.planted_source(case.dtype, case.n, case.n % 1000 + 5, amp=1.9)
    prev = F.read_slot(np.float32(2.1))                     # last step's range was smaller: the top of this tensor clips
    want = F.expect_delayed(x, case.fmt, case.q_off, prev)
    assert want["amax"] == amax and np.any((want["q"][F.BAND + case.q_off:][:case.n] & 0x7F) == F.encode(np.float32([F.FMAX[case.fmt]]), case.fmt)[0])
    s0, e = F.geometry_of(case).segs[0], case.expect
    assert (s0.wide, s0.why, s0.trips, s0.idle) == (e["wide"], e["why"], e["trips"], e["idle"]), (case.name, s0)
    got, _ = _delayed_launch(ops, dev, x, case.fmt, case.q_off, prev, case.step)
    _report(f"dg_fp8_quantize_delayed {case.name}", F.compare(got, want, case.fmt, case.name))


def test_quantize_delayed_step_word_wraps(dev):
    """step word 0xFFFFFFFF is parity 1 (slot 1 written, slot 0 read); dg_state_advance wraps it to 0: parity 0, and the maximum
    recorded a launch ago is the scale"""
    from drakegpt_amd import ops
    x1, a1 = F.planted_source(F.BF16, 8 * 1024 + 8, 11, amp=0.7)
    x2, a2 = F.planted_source(F.BF16, 8 * 1024 + 8, 12, amp=3.0)
    prev = F.read_slot(np.float32(1.5))
    state = ops.new_rng_state(1, dev, 0xFFFFFFFF)
    want = F.expect_delayed(x1, F.E4M3, 0, prev)
    got, parts2 = _delayed_launch(ops, dev, x1, F.E4M3, 0, prev, 0xFFFFFFFF, state=state)
    F.compare(got, want, F.E4M3, "step 0xFFFFFFFF")
    ops.state_advance(state)
    assert state.cpu().tolist()[2] == 0
    want2 = F.expect_delayed(x2, F.E5M2, 0, want["written"])
    got2, _ = _delayed_launch(ops, dev, x2, F.E5M2, 0, None, 0, state=state, parts2=parts2)
    F.compare(got2, want2, F.E5M2, "step 0 after the wrap")
    assert want2["scale_inv"][0] == F.scale_inv_of(F.scale_of(a1, F.FMAX[F.E5M2])) and want2["amax"] == a2


@pytest.mark.parametrize("case", F.amax_cases(), ids=lambda c: c.name)
def test_amax(dev, case):
    """dg_fp8_amax alone (n need not be a multiple of 8): every one of the 256 partial maxima, the scalar tail included"""
    from drakegpt_amd import ops
    at = F.amax_where(case.dtype, case.n, case.expect)
    x, amax = F.planted_source(case.dtype, case.n, case.n % 1000 + 7, where=at)
    ageo = F.amax_geometry(case.dtype, case.n)
    sg = ageo.segs[0]
    want = F.amax_partials(F.to_f32(x), sg, ageo)
    xbytes, parts, behind = _amax_launch(ops, dev, x)
    assert np.array_equal(xbytes, F.source_buffer(x).bytes()) and np.all(behind == GUARD)
    assert parts.max() == amax == want.max()
    F._same_bits(parts, want, case.name)
    assert np.all(parts[P - sg.idle:] == 0) if sg.idle else True


@pytest.mark.parametrize("dtype", F.DTYPES)
def test_amax_of_negative_zeros_and_of_segments(dev, dtype):
    from drakegpt_amd import ops
    z = torch.full((1003,), -0.0, dtype=F.TORCH[dtype])
    _, parts, behind = _amax_launch(ops, dev, z)
    assert np.all(parts.view(np.uint32) == 0) and np.all(behind == GUARD)                 # +0.0, not -0.0
    x, table, amaxes = F.seg_source(dtype)
    ageo = F.amax_geometry(dtype, x.numel(), table)
    xbytes, parts, behind = _amax_launch(ops, dev, x, table)
    assert np.array_equal(xbytes, F.source_buffer(x).bytes()) and np.all(behind == GUARD)
    for i, (sg, a) in enumerate(zip(ageo.segs, amaxes)):
        assert parts[i * P:(i + 1) * P].max() == a, i
        F._same_bits(parts[i * P:(i + 1) * P], F.amax_partials(F.to_f32(x), sg, ageo), f"segment {i}")
    # a table of fewer segments leaves the partials of the others alone
    _, parts, behind = _amax_launch(ops, dev, x, table[:2])
    assert np.all(behind == GUARD) and parts[P:2 * P].max() == amaxes[1]


# --------------------------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("fmt", F.FORMATS)
def test_every_finite_bf16_pattern(dev, fmt):
    """the 65280 finite bf16 patterns through the delayed entry at four scales, and through the just-in-time entry, whose amax is
    the largest finite bf16: the scale is tiny and most values land in the subnormals and on zero"""
    from drakegpt_amd import ops
    x = F.bf16_patterns()
    for name, amax, _ in F.boundary_amaxes(fmt):
        prev = F.read_slot(amax)
        want = F.expect_delayed(x, fmt, 0, prev)
        got, _ = _delayed_launch(ops, dev, x, fmt, 0, prev, 6)
        _report(f"all bf16 patterns, delayed, {fmt} {name}", F.compare(got, want, fmt, name))
    want = F.expect_quantize(x, fmt)
    view = want["q"][F.BAND:F.BAND + x.numel()]
    assert np.count_nonzero((view & 0x7F) == 0) > 30000 and np.count_nonzero(view & 0x7F) > 1000
    got = _quantize_launch(ops, dev, x, fmt)
    _report(f"all bf16 patterns, just in time, {fmt}", F.compare(got, want, fmt, "just in time"))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_rounding_boundaries_from_fp32(dev, fmt):
    """ties between neighbouring code points, their fp32 neighbours, the subnormal boundary, +-FMAX and +-0 as fp32 sources through
    the delayed entry: at power-of-two scales the product reconstructs the boundary exactly, at the other one the fp32 product
    of the model decides"""
    from drakegpt_amd import ops
    for name, amax, p2 in F.boundary_amaxes(fmt):
        x = F.boundary_sources(fmt, amax, p2)
        prev = F.read_slot(amax)
        want = F.expect_delayed(x, fmt, 0, prev)
        if p2 is not None:
            assert want["scale_inv"][0] == np.float32(1.0 / p2)
            assert np.array_equal(want["q"][F.BAND:F.BAND + x.numel()], F.encode(F.clamp(F.boundary_targets(fmt).numpy(), F.FMAX[fmt]), fmt))
        got, _ = _delayed_launch(ops, dev, x, fmt, 0, prev, 7)
        _report(f"rounding boundaries, {fmt} {name}", F.compare(got, want, fmt, name))


@pytest.mark.parametrize("fmt", F.FORMATS)
def test_non_finite_bf16_patterns(dev, fmt):
    """the 256 NaN / Inf bf16 patterns mixed into finite data, through the delayed entry with a finite scale: a NaN element is a
    NaN byte, +-Inf saturates to +-FMAX, the finite neighbours are cast as ever, the recorded maximum is not finite"""
    from drakegpt_amd import ops
    bad = F.bf16_patterns(finite=False)
    assert bad.numel() == 256 and int(torch.isinf(bad.float()).sum()) == 2
    x, _ = F.planted_source(F.BF16, 4096, 21)
    clean = x.clone()
    x[5::16] = bad
    prev = F.read_slot(np.float32(4.0))
    want = F.expect_delayed(x, fmt, 0, prev)
    view, ref = want["q"][F.BAND:F.BAND + 4096], F.expect_delayed(clean, fmt, 0, prev)["q"][F.BAND:F.BAND + 4096]
    xf = F.to_f32(x)
    top = F.encode(np.float32([F.FMAX[fmt]]), fmt)[0]
    assert F.is_nan_code(view[np.isnan(xf)], fmt).all() and np.isnan(xf).sum() == 254
    assert view[xf == np.inf].tolist() == [top] and view[xf == -np.inf].tolist() == [top | 0x80]
    assert np.array_equal(view[np.isfinite(xf)], ref[np.isfinite(xf)]) and not F.is_nan_code(view[np.isfinite(xf)], fmt).any()
    assert not np.isfinite(want["amax"])
    got, _ = _delayed_launch(ops, dev, x, fmt, 0, prev, 6)
    F.compare(got, want, fmt, "non-finite patterns")
    assert not np.isfinite(got["written"].max())


# --------------------------------------------------------------------------------------------------------------------- tiny amax
def _tiny_checks(view, zeros, sinv, fmt, what):
    """no NaN (or Inf) byte, every exact zero a zero byte (0x00, or 0x80 for a -0.0: the sign of a zero is kept), scale_inv a positive
    normal; the message says what was seen"""
    nan, sat = F.is_nan_code(view, fmt), (view & 0x7F) == F.encode(np.float32([F.FMAX[fmt]]), fmt)[0]
    seen = (f"{what}: {view.size} bytes, {int(nan.sum())} NaN, {int(sat.sum())} at +-FMAX; {int(zeros.sum())} exact zeros, of which "
            f"{int(nan[zeros].sum())} NaN; first bytes {[f'{b:02X}' for b in view[:12]]}; scale_inv {sinv!r}")
    assert not nan.any(), seen
    if fmt == F.E5M2:
        assert not np.any((view & 0x7F) == 0x7C), seen
    assert np.all((view[zeros] & 0x7F) == 0), seen
    assert np.isfinite(sinv) and sinv >= np.finfo(np.float32).tiny, seen


@pytest.mark.parametrize("entry", ["just_in_time", "delayed"])
@pytest.mark.parametrize("name,dtype,fmt,amax", F.tiny_cases(), ids=[c[0] for c in F.tiny_cases()])
def test_tiny_amax_casts_stay_finite(dev, name, dtype, fmt, amax, entry):
    """0 < amax < FMAX / FLT_MAX, exact zeros in the tensor, both entries of fp8.hip: the scale is capped at 2^126, so the
    outputs are finite, zeros are zero bytes and scale_inv = 2^-126 -- byte for byte against the model.  (Without the cap
    FMAX / amax = +Inf: every zero a NaN byte, everything else +-FMAX, scale_inv 0 -- DESIGN section 2 has the parent's output.)"""
    from drakegpt_amd import ops
    x, held = F.tiny_source(amax, dtype)
    assert held == amax
    zeros = F.to_f32(x) == 0
    if entry == "just_in_time":
        want = F.expect_quantize(x, fmt)
        got = _quantize_launch(ops, dev, x, fmt)
    else:
        prev = F.read_slot(amax)
        want = F.expect_delayed(x, fmt, 0, prev)
        got, _ = _delayed_launch(ops, dev, x, fmt, 0, prev, 6)
    _tiny_checks(got["q"][F.BAND:F.BAND + x.numel()], zeros, got["scale_inv"][0], fmt, entry)
    F.compare(got, want, fmt, entry)
    assert want["scale_inv"][0] == np.float32(2.0 ** -126)


def _codes(q8):
    return q8.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(-1)


def test_tiny_history_layernorm_fwd_fp8(dev):
    """dg_layernorm_fwd_fp8 with its history at 2^-125: columns with gamma = beta = 0 are exact zeros"""
    from drakegpt_amd import ops
    M, C = 9, 128
    g = torch.Generator().manual_seed(M + C)
    x = (torch.randn(M, C, generator=g) * 1.7 + 0.3).to(dev)
    gam, bet = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    gam[5], bet[5], gam[64:68], bet[64:68] = 0.0, 0.0, 0.0, 0.0
    n = ops.layernorm_fwd_fp8_parts(M)
    state = ops.new_rng_state(5, dev, 6)                      # step word 6: slot 0 is written, slot 1 read
    parts2 = torch.zeros(2 * n, device=dev)
    parts2[n:] = TINY_HISTORY
    y, _, _, q8, sinv = ops.layernorm_fwd_fp8(x, gam.to(dev), bet.to(dev), parts2, state)
    torch.cuda.synchronize()
    yf = F.to_f32(y.cpu())
    zeros = yf == 0
    assert zeros.reshape(M, C)[:, [5, 64, 65, 66, 67]].all()
    _tiny_checks(_codes(q8), zeros, _np(sinv)[0], F.E4M3, "layernorm_fwd_fp8")
    codes, si = F.model_cast(yf, np.float32(TINY_HISTORY), F.E4M3)
    assert np.array_equal(_codes(q8), codes) and _np(sinv)[0] == si


def test_tiny_history_gemm_nt_fp8_out(dev):
    """dg_gemm_nt with fp8_out, the bias + ReLU + sign-bit form (EPI 8), history at 2^-125: the ReLU's zeros"""
    from drakegpt_amd import ops
    M, N, K = 4096, 1024, 256                                 # 256 whole 128 x 128 tiles: the smallest shape the query accepts
    assert ops.gemm_nt_fp8_out_supported(M, N, K) and not ops.gemm_nt_fp8_out_supported(M - 128, N, K)
    g = torch.Generator().manual_seed(N + K)
    E4 = torch.float8_e4m3fn
    A = (torch.randn(M, K, generator=g) * 2.0).clamp(-448, 448).to(E4).to(dev)
    B = torch.randn(N, K, generator=g).clamp(-448, 448).to(E4).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    sa, sb = torch.tensor([0.013], device=dev), torch.tensor([0.021], device=dev)
    parts2 = torch.zeros(2 * P, device=dev)
    parts2[P:] = TINY_HISTORY                                 # step 4 is even: slot 1 is read, slot 0 written
    parts2[:P] = F.STALE
    st = ops.new_rng_state(1, dev, 4)
    q8 = torch.zeros((M, N), dtype=E4, device=dev)
    sinv = torch.zeros(1, device=dev)
    bits = ops.new_sign_bits(M, N, dev)
    f = ops.gemm_nt(A, B, torch.bfloat16, bias=bias, relu=True, sign_bits_out=bits, scale_a=sa, scale_b=sb, fp8_out=(q8, parts2, st, sinv))
    torch.cuda.synchronize()
    zeros = F.to_f32(f.cpu()) == 0
    assert 0.3 < zeros.mean() < 0.7
    _tiny_checks(_codes(q8), zeros, _np(sinv)[0], F.E4M3, "gemm_nt fp8_out")
    assert _np(sinv)[0] == np.float32(2.0 ** -126) and np.all(_codes(q8)[~zeros] == 0x7E)        # everything positive saturates
    assert np.all(_np(parts2)[P:] == np.float32(TINY_HISTORY))                                   # the read slot is untouched


def test_tiny_history_layernorm_bwd_fused_fp8(dev):
    """dg_layernorm_bwd_fused_fp8 with its history at 2^-125: rows whose dy and dresid are zero (and every dropped element)"""
    from drakegpt_amd import ops
    M, C = 300, 384
    G, site, seed, step, p = ops.FP8_AMAX_PARTS, 5, 11, 8, 0.2
    gen = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=gen)
    w, b = torch.randn(C, generator=gen), torch.randn(C, generator=gen)
    dy = torch.randn(M, C, generator=gen).bfloat16()
    dres = torch.randn(M, C, generator=gen).bfloat16()
    dy[10:40], dres[10:40] = 0.0, 0.0
    d = lambda t: t.to(dev)
    _, mean, rstd = ops.layernorm_fwd(d(x), d(w), d(b), torch.float32)
    rng = ops.new_rng_state(seed, dev, step)
    parts2 = torch.zeros(2 * P, device=dev)
    parts2[P:] = TINY_HISTORY                                 # step 8 is even: slot 1 read, slot 0 written
    parts2[:P] = F.STALE
    P1 = [torch.full((G, C), float("nan"), device=dev) for _ in range(3)]
    dx, gq, g8, sinv = ops.layernorm_bwd_fused(d(dy), d(x), d(w), mean, rstd, d(dres), P1[0], P1[1], C, G, torch.bfloat16, p, rng, site, P1[2],
                                               stream_dtype=torch.bfloat16, fp8_out=(parts2, rng))
    torch.cuda.synchronize()
    gf = F.to_f32(gq.cpu())
    zeros = gf == 0
    assert zeros.reshape(M, C)[10:40].all() and 0.25 < zeros.mean() < 0.35
    _tiny_checks(_codes(g8), zeros, _np(sinv)[0], F.E5M2, "layernorm_bwd_fused_fp8")
    codes, si = F.model_cast(gf, np.float32(TINY_HISTORY), F.E5M2)
    assert np.array_equal(_codes(g8), codes) and _np(sinv)[0] == si


def test_tiny_history_attn_fwd_fp8_out(dev):
    """dg_attn_fwd with fp8_out, history at 2^-125: one head's V rows are zero, so its output is"""
    from drakegpt_amd import ops
    B, T, NH, H = 1, 128, 2, 64
    assert ops.attn_fp8_out_supported(B, T, NH, H, torch.bfloat16)
    g = torch.Generator().manual_seed(B * 1000 + T)
    qkv = torch.randn(B * T, 3 * NH * H, generator=g).bfloat16()
    qkv[:, 2 * NH * H + H:] = 0.0                             # column blocks [Q heads | K heads | V heads]: V of head 1
    state = ops.new_rng_state(77, dev, 6)
    hist = ops.new_attn_fp8_history(torch.tensor([TINY_HISTORY], device=dev))
    o, _ = ops.attn_fwd(qkv.to(dev), B, T, NH, H, H ** -0.5, 0.0, None, 5, keep=True, fp8_out=(hist, state))
    q8, sinv = o.dg_fp8
    torch.cuda.synchronize()
    of = F.to_f32(o.cpu())
    zeros = of == 0
    assert zeros.reshape(B * T, NH * H)[:, H:].all() and not zeros.reshape(B * T, NH * H)[:, :H].all()
    _tiny_checks(_codes(q8), zeros, _np(sinv)[0], F.E4M3, "attn_fwd fp8_out")
    codes, si = F.model_cast(of, np.float32(TINY_HISTORY), F.E4M3)
    assert np.array_equal(_codes(q8), codes) and _np(sinv)[0] == si
