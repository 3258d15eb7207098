"""dg_gemm_nt per planned kernel, tile kind, K-step count and layout flip (tests/nt_run_cases.py), element by element.

Every case first asserts, from the library's own plan (dg_debug_nt_plan) of the REAL argument struct -- ops.gemm_nt_args: real
addresses and strides -- with the CU count of this device, that it runs the kernel and the flags it is named for; the same
struct is then launched.  The fp8-copy forms (EPI 8 / 9) exist on exactly 256 CUs and skip elsewhere with the plan's answer.

Every operand is a view into a larger allocation (nt_run_cases.layout).  Before every launch C, its three guard rows and the
padding of ldc are NaN; the sign-bit buffer carries 64 bytes of 0xA5 behind sign_bits_bytes; colsum_part three extra rows and
four extra columns of NaN; the fp8 copy eight columns of 0x5A; the padding of lda / ldb is NaN.  Nothing outside the written
region may change, and every element inside must be written (NaN != x).

Every case twice:
  (a) exact data -- integers, power-of-two fp8 scales, dropout p = 0.5 -- fp32 outputs BIT-EQUAL to the fp64 reference of the
      epilogue (oracle.parity.gemm_nt_epilogue_fp64, written from the description in csrc/gemm_nt_ws.h), bf16 outputs bit-equal to
      its bf16 rounding.  Emitted sign bits are decoded through the public interface alone: a consuming gemm_nt of all-ones bf16
      operands (K = 128) at the case's own (M, N) returns 128 x bit, which must equal reference > 0 everywhere, zeros included;
      on the wide tile they are decoded a second time by the generic un-prefetched instance (a bias four bytes off), so that both
      readers face the same bits.  Consumed sign bits come from an exact bias + ReLU call whose mask is known.  Column sums: the sum
      over the partial rows is bit-equal to the exact column sum; with cs_accum = 0 partial row r is bit-equal to the sum over
      rows 32 r .. 32 r + 31 of C (cs_flush((m0 >> 5) + wave row): no permutation); with cs_accum = 1 the plan's number of rows
      is written and finite.  EPI 8 / 9: with amax_prev = 112 = FMAX * 2^j the copy equals torch's cast of the exact scaled value
      byte for byte, the recorded maximum and scale_inv are exact, the slot that was read is unchanged, fp8_out_only leaves C NaN.
  (b) randn data, dropout p = 0.25: every element within P.gemm_envelope (bf16 outputs: + 1 bf16 ulp; fp32 outputs of bf16 / fp32
      operands: ulps = 0; the split contraction: P.x3_envelope, ulps = 0), compared where the sign of a ReLU is decided
      (P.mask_margin); fp32 outputs of fp8 operands keep the project's whole-tensor 4e-5 (the instruction's adder:
      test_gemm_nt_fp8_plain) -- run (a) carries their element-wise claim.

Largest error / envelope over all cases, measured on MI355X (256 CUs; a report, not a bound; DG_TEST_REPORT=1 prints them):
  gemm_nt_ws_kernel: bf16 operands 0.991 (bf16 output: the output's own rounding, as in every row below that ends near 1) and 0.014
  (fp32 output), their column sums below 0.001; e4m3 0.992 (bf16 output), fp32 output 1.4e-5 against the whole-tensor 4e-5; e5m2
  0.989, fp32 output 1.1e-5 against 4e-5, column sums 0.018; split bf16 0.057 of x3_envelope.  gemm_nt_kernel: <bf16_t,bf16_t> 0.993,
  <bf16_t,float> 0.299, <float,float> 0.417; gemm_nt_x3_kernel 0.252.  Exact data came out exact on every kernel, fp8 included,
  with A and B in [-4, 4].  The file takes 9 s on the MI355X machine (200 cases, the slowest 0.9 s).
Value-only mutants of csrc/gemm_nt_ws.h, tried one at a time on a scratch copy when this file was written: the sign-bit mask read
as (bm >> (e ^ 1)) in the interior-tile epilogue failed 44 cases (every form that consumes sign bits, and every emitting form
through its decode); cs_acc not re-zeroed after a flush failed exactly one, bf16 sign_bits + colsum at uneven-x576x128 (cs_accum = 0
with two tiles on one workgroup: the only place a flush is followed by another); the ReLU skipping element 7 in the generic
epilogue failed 14 (the EPI 0 forms with a ReLU and the emitting forms on ragged tiles); the residual added in front of the
dropout in the interior-tile epilogue failed 23, all of them bias + dropout + residual."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nt_cases as T  # noqa: E402
import nt_run_cases as R  # noqa: E402
from oracle import parity as P  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD_BYTE, Q8_BYTE, FP8_NAN = 0xA5, 0x5A, 0x7F
USE = {}
BITS = {}
FP8 = (torch.float8_e4m3fn, torch.float8_e5m2)


def _ops():
    from drakegpt_amd import ops
    return ops


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _note(key, use):
    USE[key] = max(USE.get(key, 0.0), use)
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[nt] envelope use {key}: {use:.3f} (largest so far {USE[key]:.3f})", flush=True)


def guarded(dev, view, dtype, data=None, fill=NAN):
    """(allocation, the view into it): the allocation filled with ``fill`` (fp8: the NaN byte), the view with ``data``"""
    if dtype in FP8 or dtype == torch.uint8:
        raw = torch.full((view.total,), fill if dtype == torch.uint8 else FP8_NAN, dtype=torch.uint8, device=dev)
        if data is not None:
            raw.as_strided((view.rows, view.cols), (view.ld, 1), view.off).copy_(data.view(torch.uint8).to(dev))
        buf = raw.view(dtype)
    else:
        buf = torch.full((view.total,), fill, dtype=dtype, device=dev)
        if data is not None:
            buf.as_strided((view.rows, view.cols), (view.ld, 1), view.off).copy_(data.reshape(view.rows, view.cols).to(dev))
    return buf, buf.as_strided((view.rows, view.cols), (view.ld, 1), view.off)


def split_view(host, view):
    """(the [rows, cols] view of a host copy of an allocation, the mask of everything else in it)"""
    rest = torch.ones(view.total, dtype=torch.bool)
    rest.as_strided((view.rows, view.cols), (view.ld, 1), view.off).fill_(False)
    return host.as_strided((view.rows, view.cols), (view.ld, 1), view.off), rest


def bits_buffer(dev, M, N):
    n = R.sign_bits_bytes(M, N)
    buf = torch.full((n + 64,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    return buf, buf[:n]


def guard_ok(buf):
    return bool((buf[-64:] == GUARD_BYTE).all())


def known_bits(dev, M, N):
    """sign bits of a known mask for the consuming cases of this shape (nt_run_cases.mask_operands), emitted once"""
    if (M, N) not in BITS:
        A, B, bias, mask = R.mask_operands(M, N)
        buf, bits = bits_buffer(dev, M, N)
        _ops().gemm_nt(A.to(dev), B.to(dev), torch.bfloat16, bias=bias.to(dev), relu=True, sign_bits_out=bits)
        BITS[(M, N)] = (buf, bits, mask)
    return BITS[(M, N)]


def decode_bits(dev, bits, M, N, unprefetched=False):
    """the mask behind ``bits`` through the public interface: ones . ones^T (K = 128) under sign_bits is 128 x bit"""
    ops = _ops()
    one = lambda rows: torch.ones((rows, 128), dtype=torch.bfloat16, device=dev)
    kw = {}
    if unprefetched:                                                  # a bias four bytes off: the generic EPI 0 instance reads the bits
        kw["bias"] = torch.zeros(N + 1, device=dev)[1:]
    a, out = ops.gemm_nt_args(one(M), one(N), torch.bfloat16, sign_bits=bits, **kw)
    pl = T.plan_of(a, 0, 0)
    assert (pl.pf, pl.epi) == ((0, 0) if unprefetched else (1, 4)), pl
    ops.check(ops.lib.dg_gemm_nt(C.byref(a), ops._stream()), "dg_gemm_nt")
    got = out.float().cpu()
    assert bool(((got == 0) | (got == 128)).all())
    return got == 128


def first(bad):
    return tuple(int(i) for i in bad.nonzero()[0])


def run_case(dev, case, kind, ncu):
    ops = _ops()
    M, N, K, opts = case.M, case.N, case.K, case.opts
    exact = kind == "exact"
    what = f"{case.name} [{kind}]"
    d = R.operands(case, kind)
    sign_buf = sign_in = sign_mask = None
    if "sign_bits" in opts:
        sign_buf, sign_in, sign_mask = known_bits(dev, M, N)
    r = R.reference(case, d, sign_mask)
    if exact:
        R.exact_conditions(case, d, r)
    in_dt, out_dt = R.TORCH[case.ind], R.TORCH[case.outd]
    rows = ops.gemm_nt_colsum_rows(out_dt, M, N, K, in_dtype=in_dt) if "colsum" in opts else 0
    lay = R.layout(case, rows)
    bufs, v = {}, {}
    for k, dt in (("A", in_dt), ("B", R.TORCH[R.E4M3] if case.fp8 else in_dt), ("C", out_dt), ("bias", torch.float32),
                  ("residual", torch.float32), ("relu_mask", in_dt), ("colsum_part", torch.float32)):
        if k in lay:
            bufs[k], v[k] = guarded(dev, lay[k], dt, d.get(k))
    kw = dict(out=v["C"], relu="relu" in opts, split=case.ind == R.X3)
    if "bias" in opts:
        kw["bias"] = v["bias"].view(-1)
    for k in ("residual", "relu_mask", "colsum_part"):
        if k in lay:
            kw[k] = v[k]
    if d["p"]:
        kw.update(dropout_p=d["p"], rng_state=ops.new_rng_state(R.SEED, dev, R.STEP), site=R.SITE)
    if case.fp8:
        kw.update(scale_a=d["scale_a"].to(dev), scale_b=d["scale_b"].to(dev))
    if sign_in is not None:
        kw["sign_bits"] = sign_in
    out_buf = None
    if "sign_bits_out" in opts:
        out_buf, kw["sign_bits_out"] = bits_buffer(dev, M, N)
    if "fp8_out" in opts:
        n = ops.FP8_AMAX_PARTS
        bufs["q8"], v["q8"] = guarded(dev, lay["fp8_out"], torch.uint8, fill=Q8_BYTE)
        parts2 = torch.full((2 * n,), 123.0, device=dev)              # stale values in the slot to be written
        parts2[n:] = torch.rand(n, generator=R._gen(case.name, "amax")).to(dev) * R.AMAX_PREV * 0.5
        parts2[n + 17] = R.AMAX_PREV
        before = parts2.clone()
        sinv = torch.full((1,), NAN, device=dev)
        kw["fp8_out"] = (v["q8"].view(in_dt), parts2, ops.new_rng_state(1, dev, R.FP8_STEP), sinv)
        kw["fp8_out_only"] = "fp8_out_only" in opts
    a, out = ops.gemm_nt_args(v["A"], v["B"], out_dt, **kw)
    # ---- the plan of this very struct
    pl = T.plan_of(a, 0, 0)
    if "fp8_out" in opts and ncu != 256:
        assert pl.rc != 0 and not pl.fp8_out_ok, pl
        pytest.skip(f"the fp8 copy of the output is offered on exactly 256 CUs, this device has {ncu}: dg_gemm_nt answers {pl.rc}")
    R.check_plan(case, pl, ncu)
    if "colsum" in opts:
        assert pl.colsum_rows == rows > 0
    ops.check(ops.lib.dg_gemm_nt(C.byref(a), ops._stream()), "dg_gemm_nt")
    torch.cuda.synchronize()

    # ---- C inside its guard band
    full = bufs["C"].cpu()
    host, rest = split_view(full, lay["C"])
    assert bool(torch.isnan(full[rest]).all()), f"{what}: written outside C [M, N] (in front, the padding of ldc, the rows behind M)"
    env, pre_env = R.envelopes(case, d, r)
    decided = None
    if not exact and ("relu" in opts or "sign_bits_out" in opts):
        decided = P.mask_margin(r["pre"], pre_env)
    bf16_out = case.outd == R.BF16
    if "fp8_out_only" in opts:
        assert bool(torch.isnan(full).all()), f"{what}: fp8_out_only wrote C"
    elif exact:
        want = P.rb(r["out"]) if bf16_out else r["out"]
        bad = host.double() != want                                   # (NaN != x: an unwritten element counts)
        assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact result, first at {first(bad)}: "
                                     f"got {host[first(bad)].item()}, want {want[first(bad)].item()}")
    elif case.fp8 and not bf16_out:
        e = P.rel(host, r["out"])
        assert e < 4e-5, (what, e)
        _note(f"{case.family} > f32, whole-tensor error / 4e-5", e / 4e-5)
    else:
        _note(f"{case.family} > {R.FAMILY[case.outd]}", P.assert_within_rounding(host, r["out"], env, ulps=1 if bf16_out else 0, name=what, where=decided))

    # ---- emitted sign bits
    if out_buf is not None:
        assert guard_ok(out_buf), f"{what}: bytes behind sign_bits_bytes were written"
        for unpf in ((False, True) if N % 192 == 0 else (False,)):
            got = decode_bits(dev, kw["sign_bits_out"], M, N, unpf)
            bad = got != r["bit"]
            if decided is not None:
                bad &= decided
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} emitted sign bits differ from reference > 0 ({'un-' if unpf else ''}prefetched reader), first at {first(bad)}"
        assert guard_ok(out_buf)
    if sign_buf is not None:
        assert guard_ok(sign_buf)

    # ---- column sums
    if "colsum" in opts:
        cs, rest = split_view(bufs["colsum_part"].cpu(), lay["colsum_part"])
        assert bool(torch.isnan(bufs["colsum_part"].cpu()[rest]).all()), f"{what}: written outside colsum_part [{rows}, N]"
        assert bool(torch.isfinite(cs).all()), f"{what}: {int((~torch.isfinite(cs)).sum())} elements of the {rows} partial rows unwritten or not finite"
        total = cs.double().sum(0)
        if exact:
            assert torch.equal(total, r["colsum"]), f"{what}: column sums differ in {int((total != r['colsum']).sum())} columns"
            if not pl.cs_accum:
                per32 = r["out"].view(M // 32, 32, N).sum(1)
                bad = cs.double() != per32
                assert not bool(bad.any()), f"{what}: partial row r is not the sum over rows 32 r .. 32 r + 31 of C, first at {first(bad)}"
        else:
            # M values of their own envelope each, summed in fp32: M roundings on a running sum bounded by sum |v|
            cs_env = env.sum(0) + M * 2.0 ** -24 * r["out"].abs().sum(0)
            _note(f"{case.family} column sums", P.assert_within_rounding(total.view(1, N), r["colsum"].view(1, N), cs_env.view(1, N), ulps=0, name=what + " column sums"))

    # ---- the fp8 copy
    if "fp8_out" in opts:
        n, fmax = ops.FP8_AMAX_PARTS, R.FMAX[case.ind]
        q8, rest = split_view(bufs["q8"].cpu(), lay["fp8_out"])
        assert bool((bufs["q8"].cpu()[rest] == Q8_BYTE).all()), f"{what}: written outside the fp8 copy [M, N]"
        assert sinv.item() == R.AMAX_PREV / fmax and torch.equal(parts2[n:], before[n:])
        rec = parts2[:n].cpu()
        top = r["out"].abs().max().item()
        assert top <= R.AMAX_PREV and rec.min().item() >= 0.0                         # no clipping
        if exact:
            assert rec.max().item() == top
            want8 = (r["out"] * (fmax / R.AMAX_PREV)).float().to(in_dt).view(torch.uint8)
            bad = q8 != want8
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} bytes of the fp8 copy differ from the cast of the exact scaled value, first at {first(bad)}"
        else:
            assert abs(rec.max().item() - top) <= env.max().item()
            got = q8.view(in_dt).float().double() * sinv.item()
            half, tiny = (2.0 ** -4, 2.0 ** -10) if case.ind == R.E4M3 else (2.0 ** -3, 2.0 ** -17)
            tol = (r["out"].abs() + env) * (half + 1e-6) + sinv.item() * tiny + env
            bad = ~((got - r["out"]).abs() <= tol)
            assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements of the fp8 copy off by more than half an fp8 ulp, first at {first(bad)}"


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_gemm_nt_case(dev, name):
    ncu = _ncu(dev)
    case = {c.name: c for c in R.run_cases(ncu)}[name]
    for kind in ("exact", "randn"):
        run_case(dev, case, kind, ncu)
