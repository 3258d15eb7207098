"""drakegpt_amd/csrc/layernorm.hip, instance by instance: the scalar path (C % 4 != 0, C > 2048, a misaligned operand), every
width class of the vector path at a full and at a ragged width, workgroups without rows, fewer rows than waves, the
prefetching bf16-stream instance at the ends of its chunks, and the two fp8 forms at small and ragged row counts -- each against
fp64 on the same operands.  The cases and the restated dispatch live in tests/layernorm_cases.py (held against the list of
template instances by tests/test_layernorm_cases_host.py); a case's id names its entry point, width, dtypes and options.

Checks, in this order:
  * at C >= 32 the whole-tensor tolerances of tests/test_gpu_ops.py: forward 1e-6 fp32 / 4e-3 bf16, backward 2e-6 (bf16 stores
    3e-3), reduced partial sums 3e-6;
  * every ROW: oracle.parity.rowwise_rel against max(that tolerance, 4 x the worst row of the fp32 CPU model of the kernel's
    formulas, oracle.parity.layernorm_model) -- for the backward's outputs at C < 32 the model alone; mean and rstd of every
    row inside assert_layernorm_stats; bf16 stores inside one rounding (assert_within_rounding, single_rounding_envelope);
    dropped elements of g exact zeros;
  * every COLUMN of the reduced partials: |got - ref| <= 4 x (model's worst column error / sum |term|) x sum |term|;
  * the partial buffers arrive filled with NaN at part_stride = C + 8: rows of workgroups without rows must come back as exact
    zeros, columns C .. C + 7 must still hold NaN; the fp8 history slot being written arrives as NaN and must come back finite,
    and 0 where a workgroup had no rows.
The model's worst row / column is taken over all ROWS_MAX rows (all row counts) of a case's operands: a reference-side number.

Measured on MI355X with DG_TEST_REPORT=1 (worst over a group's cases and row counts; kernel / model = worst row rel. error, or
for sums the worst column error / sum |term|; use = largest error / bound):

  per width: quantity kernel/model/use (mean, rstd: use of assert_layernorm_stats' bound); +4B: an operand 4 bytes off a 16-byte
  boundary (the scalar path at a vector width)
  bwd
    4: dx f32 9.7e-7/1.4e-6/.18  dgamma 1.5e-7/1.5e-7/.25  dbeta 5.2e-8/5.2e-8/.25
    100: dx f32 6.0e-8/9.7e-8/.03  dgamma 3.4e-7/3.4e-7/.25  dbeta 1.0e-7/1.0e-7/.25
    256: dx f32 5.3e-8/8.0e-8/.03  dgamma 5.8e-6/1.3e-5/.12  dbeta 1.1e-7/1.1e-7/.55
    260: dx f32 9.4e-8/1.7e-7/.05  dgamma 7.2e-6/7.2e-6/.25  dbeta 9.8e-8/9.8e-8/.25
    512: dx f32 4.7e-8/7.6e-8/.02  dgamma 1.4e-6/1.3e-6/.27  dbeta 9.1e-8/9.1e-8/.25
    516: dx f32 4.7e-8/8.0e-8/.02  dgamma 2.1e-5/3.1e-5/.17  dbeta 1.2e-7/1.2e-7/.25
    768: dx f32 4.7e-8/7.4e-8/.02  dgamma 2.9e-6/9.7e-6/.08  dbeta 1.0e-7/1.0e-7/.25
    772: dx f32 4.4e-8/8.0e-8/.02  dgamma 6.1e-5/1.2e-4/.13  dbeta 1.0e-7/1.1e-7/.25
    1020: dx f32 4.5e-8/8.6e-8/.02  dgamma 1.3e-6/1.3e-6/.25  dbeta 1.3e-7/1.3e-7/.25
    1024: dx f32 4.4e-8/7.6e-8/.02  dgamma 7.1e-6/7.1e-6/.25  dbeta 1.1e-7/1.1e-7/.25
    1028: dx f32 4.7e-8/8.1e-8/.02  dgamma 3.2e-6/7.7e-6/.10  dbeta 1.1e-7/1.1e-7/.25
    1280: dx f32 4.4e-8/8.0e-8/.02  dgamma 1.5e-4/1.5e-4/.25  dbeta 1.0e-7/1.0e-7/.25
    1600: dx f32 8.4e-8/1.6e-7/.04  dgamma 1.1e-5/1.1e-5/.25  dbeta 1.1e-7/1.1e-7/.25
    2044: dx f32 4.6e-8/7.3e-8/.02  dgamma 7.5e-7/8.5e-7/.22  dbeta 1.1e-7/1.1e-7/.25
    2048: dx f32 4.6e-8/7.7e-8/.02  dgamma 7.3e-4/7.3e-4/.25  dbeta 1.4e-7/1.4e-7/.25
  bwd scalar
    1: dx f32 3.2e-12/3.2e-12/.25  dgamma 0.0e+00/.0e+00/.00  dbeta 2.7e-8/1.3e-8/.51
    3: dx f32 2.8e-6/2.7e-6/.26  dgamma 1.1e-6/1.1e-6/.25  dbeta 1.8e-8/3.2e-8/.14
    30: dx f32 1.4e-7/2.0e-7/.17  dgamma 6.0e-7/2.0e-6/.07  dbeta 4.2e-8/6.9e-8/.15
    63: dx f32 6.9e-8/8.1e-8/.04  dgamma 1.2e-7/7.8e-7/.04  dbeta 1.0e-7/1.0e-7/.25
    65: dx f32 7.5e-8/1.1e-7/.04  dgamma 6.7e-7/6.7e-7/.25  dbeta 6.3e-8/4.9e-8/.32
    101: dx f32 5.8e-8/8.4e-8/.03  dgamma 7.3e-7/4.0e-6/.05  dbeta 7.7e-8/7.7e-8/.25
    384+4B: dx f32 5.2e-8/9.1e-8/.03  dgamma 4.5e-6/8.9e-6/.13  dbeta 9.9e-8/9.9e-8/.25
    510: dx f32 5.2e-8/8.2e-8/.03  dgamma 2.8e-6/2.8e-6/.25  dbeta 9.1e-8/9.1e-8/.25
    768+4B: dx f32 4.9e-8/7.4e-8/.03  dgamma 2.9e-6/9.7e-6/.07  dbeta 1.0e-7/1.0e-7/.25
    1001: dx f32 8.1e-8/1.5e-7/.04  dgamma 5.3e-7/5.3e-7/.25  dbeta 1.1e-7/1.1e-7/.25
    2046: dx f32 4.6e-8/6.8e-8/.02  dgamma 3.1e-6/3.0e-6/.26  dbeta 1.2e-7/1.2e-7/.25
    2048+4B: dx f32 4.6e-8/7.7e-8/.02  dgamma 7.3e-4/7.3e-4/.25  dbeta 1.4e-7/1.4e-7/.25
  fused
    4: dx f32 9.7e-7/1.6e-6/.18  g f32 9.7e-7/1.5e-6/.33  dgamma 1.5e-7/1.5e-7/.25  dbeta 5.2e-8/5.2e-8/.25  gbias 1.5e-6/1.3e-6/.40  g bf16 3.5e-3/3.5e-3/.25
    100: dx f32 1.2e-7/1.6e-7/.06  g f32 1.1e-7/1.6e-7/.06  dgamma 3.4e-7/3.4e-7/.25  dbeta 1.0e-7/1.0e-7/.25  gbias 3.9e-6/2.9e-6/.50  g bf16 2.5e-3/2.5e-3/.25
    256: dx f32 1.0e-7/1.6e-7/.05  g f32 9.1e-8/1.5e-7/.05  dgamma 5.8e-6/1.3e-5/.12  dbeta 1.1e-7/1.1e-7/.55  gbias 4.0e-6/7.0e-6/.48  g bf16 2.3e-3/2.3e-3/.25
    260: dx f32 9.4e-8/1.7e-7/.05  g f32 9.4e-8/1.7e-7/.05  dgamma 7.2e-6/7.2e-6/.25  dbeta 9.8e-8/9.8e-8/.25  gbias 4.7e-6/9.6e-6/.17  g bf16 2.2e-3/2.2e-3/.25
    512: dx f32 8.8e-8/1.7e-7/.04  g f32 8.8e-8/1.5e-7/.04  dgamma 1.4e-6/1.3e-6/.27  dbeta 9.1e-8/9.1e-8/.25  gbias 8.6e-4/2.8e-3/.11  g bf16 2.1e-3/2.1e-3/.25
    516: dx f32 9.1e-8/1.7e-7/.05  g f32 9.1e-8/1.7e-7/.05  dgamma 2.1e-5/3.1e-5/.17  dbeta 1.2e-7/1.2e-7/.25  gbias 1.2e-5/9.9e-6/.31  g bf16 2.1e-3/2.1e-3/.25
    768: dx f32 8.6e-8/1.5e-7/.04  g f32 8.6e-8/1.5e-7/.04  dgamma 2.9e-6/9.7e-6/.08  dbeta 1.0e-7/1.0e-7/.25  gbias 5.7e-3/6.7e-3/.70  g bf16 2.0e-3/2.0e-3/.25
    772: dx f32 8.4e-8/1.9e-7/.04  g f32 8.4e-8/1.9e-7/.04  dgamma 6.1e-5/1.2e-4/.13  dbeta 1.0e-7/1.1e-7/.25  gbias 5.7e-6/1.7e-5/.12  g bf16 2.0e-3/2.0e-3/.25
    1020: dx f32 8.6e-8/1.8e-7/.04  g f32 8.6e-8/1.8e-7/.04  dgamma 1.3e-6/1.3e-6/.25  dbeta 1.3e-7/1.3e-7/.25  gbias 2.2e-5/1.9e-5/.42  g bf16 2.0e-3/2.0e-3/.25
    1024: dx f32 8.4e-8/1.6e-7/.04  g f32 8.3e-8/1.5e-7/.04  dgamma 7.1e-6/7.1e-6/.25  dbeta 1.1e-7/1.1e-7/.25  gbias 9.3e-6/2.2e-5/.16  g bf16 2.0e-3/2.0e-3/.25
  fused bf16 stream
    100: dx bf16 2.2e-3/2.5e-3/.25  g bf16 2.2e-3/2.5e-3/.25  dgamma 1.7e-7/2.1e-7/.20  dbeta 0.0e+00/.0e+00/.00  gbias 1.6e-7/2.4e-7/.24
    256: dx bf16 2.3e-3/2.3e-3/.25  g bf16 2.3e-3/2.3e-3/.25  dgamma 1.4e-7/1.7e-7/.21  dbeta 1.4e-8/1.4e-8/.25  gbias 2.2e-7/2.7e-7/.25
    384: dx bf16 1.9e-3/2.3e-3/.25  g bf16 2.0e-3/2.3e-3/.25  dgamma 1.2e-7/2.6e-7/.11  dbeta 2.2e-8/2.2e-8/.25  gbias 7.0e-7/5.0e-7/.35
    512: dx bf16 1.9e-3/2.0e-3/.25  g bf16 2.0e-3/2.0e-3/.25  dgamma 1.5e-7/5.3e-7/.07  dbeta 1.7e-8/1.7e-8/.25  gbias 9.3e-7/9.3e-7/.25
    516: dx bf16 2.0e-3/2.1e-3/.24  g bf16 2.3e-3/2.3e-3/.25  dgamma 2.2e-7/6.0e-7/.09  dbeta 9.8e-9/9.8e-9/.25  gbias 5.5e-7/3.2e-7/.43
    768: dx bf16 1.9e-3/2.0e-3/.25  g bf16 2.0e-3/2.1e-3/.25  dgamma 1.7e-7/3.1e-7/.14  dbeta 1.7e-8/3.7e-8/.11  gbias 1.3e-6/1.3e-6/.50
    772: dx bf16 1.9e-3/2.0e-3/.24  g bf16 2.0e-3/2.0e-3/.24  dgamma 1.4e-7/2.2e-7/.16  dbeta 1.4e-8/1.4e-8/.25  gbias 1.2e-6/1.8e-6/.19
    1024: dx bf16 1.9e-3/1.9e-3/.25  g bf16 2.0e-3/2.0e-3/.25  dgamma 1.9e-7/1.7e-7/.28  dbeta 1.1e-8/1.1e-8/.25  gbias 2.7e-6/7.3e-6/.18
  fused fp8
    260: dx f32 4.8e-8/7.3e-8/.02  g bf16 2.0e-3/2.0e-3/.25  dgamma 4.9e-8/6.8e-8/.18  dbeta 1.3e-8/1.3e-8/.26  gbias 3.7e-8/5.6e-8/.22
    1024: dx f32 4.4e-8/7.6e-8/.02  g bf16 1.8e-3/1.8e-3/.25  dgamma 7.0e-8/7.1e-8/.25  dbeta 8.6e-9/7.7e-9/.31  gbias 5.7e-8/5.5e-8/.26
  fused fp8 bf16 stream
    260: dx bf16 1.9e-3/1.9e-3/.25  g bf16 1.9e-3/2.0e-3/.24  dgamma 4.9e-8/6.8e-8/.18  dbeta 1.3e-8/1.3e-8/.26  gbias 5.7e-8/4.1e-8/.35
    1024: dx bf16 1.8e-3/1.8e-3/.25  g bf16 1.8e-3/1.8e-3/.25  dgamma 7.0e-8/7.1e-8/.25  dbeta 8.6e-9/7.7e-9/.31  gbias 9.3e-8/5.2e-8/.44
  fwd
    4: y f32 3.2e-7/3.3e-7/.24  mean .36  rstd .18  y bf16 3.0e-3/3.0e-3/.25
    100: y f32 9.9e-8/1.2e-7/.10  mean .29  rstd .10  y bf16 2.3e-3/2.3e-3/.25
    256: y f32 8.8e-8/1.3e-7/.09  mean .17  rstd .09  y bf16 2.0e-3/2.0e-3/.25
    260: y f32 9.3e-8/1.2e-7/.09  mean .23  rstd .12  y bf16 2.0e-3/2.0e-3/.25
    512: y f32 1.1e-7/1.1e-7/.11  mean .17  rstd .10  y bf16 2.0e-3/2.0e-3/.25
    516: y f32 8.2e-8/1.2e-7/.08  mean .22  rstd .09  y bf16 2.0e-3/2.0e-3/.25
    768: y f32 8.8e-8/1.0e-7/.09  mean .24  rstd .10  y bf16 1.9e-3/1.9e-3/.25
    772: y f32 8.4e-8/1.4e-7/.08  mean .22  rstd .09  y bf16 1.9e-3/1.9e-3/.25
    1020: y f32 1.1e-7/1.3e-7/.11  mean .30  rstd .12  y bf16 1.9e-3/1.9e-3/.25
    1024: y f32 9.0e-8/1.1e-7/.09  mean .22  rstd .09  y bf16 1.9e-3/1.9e-3/.25
    1028: y f32 8.9e-8/1.1e-7/.09  mean .21  rstd .09  y bf16 1.8e-3/1.8e-3/.25
    1280: y f32 9.5e-8/1.2e-7/.10  mean .21  rstd .10  y bf16 1.8e-3/1.8e-3/.25
    1600: y f32 8.4e-8/1.1e-7/.08  mean .22  rstd .09  y bf16 1.8e-3/1.8e-3/.25
    2044: y f32 7.7e-8/1.1e-7/.08  mean .21  rstd .08  y bf16 1.8e-3/1.8e-3/.25
    2048: y f32 8.5e-8/1.2e-7/.09  mean .18  rstd .09  y bf16 1.8e-3/1.8e-3/.25
  fwd scalar
    1: y f32 0.0e+00/.0e+00/.00  mean .00  rstd .18  y bf16 3.1e-4/3.1e-4/.08
    3: y f32 8.4e-7/3.8e-7/.55  mean .53  rstd .22  y bf16 3.6e-3/3.6e-3/.25
    30: y f32 1.1e-7/1.1e-7/.11  mean .51  rstd .15  y bf16 2.5e-3/2.5e-3/.25
    63: y f32 1.1e-7/1.2e-7/.11  mean .32  rstd .15  y bf16 2.4e-3/2.4e-3/.25
    65: y f32 1.0e-7/1.2e-7/.10  mean .32  rstd .12  y bf16 2.4e-3/2.4e-3/.25
    101: y f32 9.5e-8/1.2e-7/.10  mean .27  rstd .10  y bf16 2.3e-3/2.3e-3/.25
    384+4B: y f32 1.0e-7/1.4e-7/.10  mean .21  rstd .11  y bf16 1.9e-3/1.9e-3/.25
    510: y f32 1.2e-7/1.2e-7/.12  mean .28  rstd .13  y bf16 2.0e-3/2.0e-3/.25
    1001: y f32 9.3e-8/1.1e-7/.09  mean .25  rstd .09  y bf16 1.8e-3/1.8e-3/.25
    2046: y f32 8.1e-8/1.0e-7/.08  mean .21  rstd .08  y bf16 1.8e-3/1.8e-3/.25
    4096: y f32 7.9e-8/1.1e-7/.08  mean .18  rstd .07  y bf16 1.8e-3/1.8e-3/.25
  fwd_fp8
    4: y bf16 2.9e-3/3.0e-3/.24
    100: y bf16 2.2e-3/2.3e-3/.24
    256: y bf16 2.0e-3/2.0e-3/.25
    260: y bf16 2.0e-3/2.0e-3/.25
    512: y bf16 1.8e-3/2.0e-3/.24
    516: y bf16 2.0e-3/2.0e-3/.25
    768: y bf16 1.8e-3/1.9e-3/.24
    772: y bf16 1.8e-3/1.9e-3/.24
    1024: y bf16 1.8e-3/1.9e-3/.24
  largest use: 0.70
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layernorm_cases as L  # noqa: E402
from oracle import parity as P  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16 = L.F32, L.BF16
TORCH = L.TORCH
TOL_FWD = {F32: 1e-6, BF16: 4e-3}
TOL_BWD = {F32: 2e-6, BF16: 3e-3}
TOL_SUM = 3e-6
E5 = torch.float8_e5m2
E5_MAX, E4_MAX = 57344.0, 448.0
PAD = 8                                    # part_stride = C + PAD


def _ops():
    from drakegpt_amd import ops
    return ops


def _note(c, what, kernel, model, use):
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[layernorm] {c.id} | {what} | kernel {kernel:.3e} | model {model:.3e} | use {use:.3f}", flush=True)


def _put(t, dev, misaligned=False):
    """t on the device; misaligned: 4 bytes past a 16-byte boundary, as a contiguous view"""
    if not misaligned:
        return t.to(dev)
    k = 4 // t.element_size()
    v = torch.empty(t.numel() + k, dtype=t.dtype, device=dev)[k:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _nan(dev, *shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _use(err, bound):
    return err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))


def check_rows(c, what, got, ref, model, tol, cancels):
    """got [M, C] (device) against the first M rows of ref [ROWS_MAX, C]; model: the fp32 model's tensor, rounded here where
    the kernel stores bf16.  Whole tensor first (C >= 32), then every row, then (bf16) every element."""
    M, C = got.shape
    bf = got.dtype == torch.bfloat16
    bound, m = P.layernorm_row_bound(P.rb(model) if bf else model, ref, C, tol, cancels)
    r = ref[:M]
    assert bool(torch.isfinite(got).all()), f"{c.id} M={M} {what}: non-finite elements"
    if C >= 32:
        whole = P.rel(got, r)
        assert whole < tol, f"{c.id} M={M} {what}: whole-tensor error {whole:.3e} >= {tol:.1e}"
    e = P.rowwise_rel(got, r, C)
    worst = int(e.argmax())
    k = e[worst].item()
    _note(c, f"{what} rows M={M}", k, m, _use(k, bound))
    assert k <= bound, (f"{c.id} M={M} {what}: worst row {worst} has error {k:.3e} > {bound:.3e} (model's worst row {m:.3e}); "
                        f"{int((e > bound).sum())} of {M} rows over the bound, first {int((e > bound).nonzero()[0])}")
    if bf:
        P.assert_within_rounding(got, r, P.single_rounding_envelope(r, C), 1, f"{c.id} M={M} {what}")


def column_ratio(model_terms, ref_terms, rows):
    """the model's worst column error / sum |term| over the row counts of a case"""
    worst = 0.0
    for M in rows:
        worst = max(worst, P.layernorm_column_bound(model_terms[:M].sum(0), ref_terms[:M].sum(0), ref_terms[:M])[1])
    return worst


def check_partials(c, what, part, G, M, C, ref_terms, ratio, dev):
    """the partial rows themselves (finite where a workgroup owns rows, exact zeros where it owns none, NaN beyond column C),
    then their reduction per column"""
    ops = _ops()
    rows_per = -(-M // G)
    used = -(-M // rows_per)
    p = part.cpu()
    assert bool(torch.isnan(p[:, C:]).all()), f"{c.id} M={M} G={G} {what}: columns C .. C + {PAD - 1} of the partial rows were written"
    assert bool(torch.isfinite(p[:used, :C]).all()), f"{c.id} M={M} G={G} {what}: a partial row of a workgroup with rows is not finite"
    bad = (p[used:, :C] != 0).any(1).nonzero()
    assert bad.numel() == 0, f"{c.id} M={M} G={G} {what}: partial row {used + int(bad[0])} of a workgroup without rows is not zero ({G - used} such rows)"
    out = _nan(dev, C)
    ops.reduce_partials(part, C + PAD, G, out, C)
    ref = ref_terms[:M].sum(0)
    if C >= 32:
        whole = P.rel(out, ref)
        assert whole < TOL_SUM, f"{c.id} M={M} G={G} {what}: whole-tensor error {whole:.3e} >= {TOL_SUM:.1e}"
    mag = ref_terms[:M].abs().sum(0).clamp_min(1e-300)
    err = (P.f64(out) - ref).abs()
    bound = P.LN_MARGIN * ratio * mag
    col = int((err - bound).argmax())
    k = (err / mag).max().item()
    _note(c, f"{what} columns M={M}", k, ratio, _use(k, P.LN_MARGIN * ratio))
    assert bool((err <= bound).all()), (f"{c.id} M={M} G={G} {what}: column {col} is off by {err[col].item():.3e} > {bound[col].item():.3e} "
                                        f"(sum |term| {mag[col].item():.3e}); {int((err > bound).sum())} of {C} columns over the bound")


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", L.FWD_CASES, ids=lambda c: c.id)
def test_forward(dev, c):
    ops = _ops()
    C, op = c.C, L.operands(c.C)
    ref, mod = L.forward_reference(C)
    x, w, b = _put(op["x"], dev, c.misaligned == "x"), _put(op["w"], dev, c.misaligned == "gamma"), _put(op["b"], dev)
    for M in c.rows:
        y, mean, rstd = ops.layernorm_fwd(x[:M], w, b, TORCH[c.out])
        assert y.shape == (M, C) and y.dtype == TORCH[c.out]
        check_rows(c, "y", y, ref["y"], mod["y"], TOL_FWD[c.out], False)
        um, ur = P.assert_layernorm_stats(mean, rstd, op["x"][:M], ref["mean"][:M], ref["std"][:M], ref["xhat"][:M], f"{c.id} M={M}")
        _note(c, f"mean M={M}", um, 0.0, um)
        _note(c, f"rstd M={M}", ur, 0.0, ur)


# ---------------------------------------------------------------------------------------------------------------------
# backward: dg_layernorm_bwd, dg_layernorm_bwd_fused (fp32 stream and the prefetching bf16 stream)
# ---------------------------------------------------------------------------------------------------------------------
def _stats(C, dev, M=L.ROWS_MAX):
    """mean / rstd as the backward receives them: the fp64 statistics rounded to fp32 (the forward has its own tests)"""
    ref = L.forward_reference(C)[0]
    return ref["mean"].view(-1).float().to(dev), ref["rstd"].view(-1).float().to(dev)


def _backward_case(dev, c, fp8=None):
    ops = _ops()
    C, op = c.C, L.operands(c.C)
    fused = c.entry != "bwd"
    ref, mod = L.backward_reference(C, c.dy, c.stream, c.dresid, c.p)
    mis = c.misaligned
    x, w = _put(op["x"], dev, mis == "x"), _put(op["w"], dev, mis == "gamma")
    dy = _put(op["dy"].to(TORCH[c.dy]), dev, mis == "dy")
    dres = op["dres"].to(TORCH[c.stream]).to(dev) if c.dresid else None
    mean, rstd = _stats(C, dev)
    rng = ops.new_rng_state(L.SEED, dev, L.STEP)
    keep = L.keep_scale(C, c.p)
    sums = [("dgamma", "dgamma_terms"), ("dbeta", "dbeta_terms")] + ([("gbias", "gbias_terms")] if c.gbias else [])
    ratios = {n: column_ratio(mod[t], ref[t], [M for M, _ in c.rows]) for n, t in sums}
    tol_dx = TOL_BWD[c.stream]
    for M, G in c.rows:
        parts = {n: _nan(dev, G, C + PAD) for n, _ in sums}
        dr = None if dres is None else dres[:M]
        if not fused:
            dx_out = _put(torch.full((M, C), float("nan")), dev, True) if mis == "dx" else None
            dx = ops.layernorm_bwd(dy[:M], x[:M], w, mean[:M], rstd[:M], dr, parts["dgamma"], parts["dbeta"], C + PAD, G, dx=dx_out)
            g = None
        else:
            dx, g = ops.layernorm_bwd_fused(dy[:M], x[:M], w, mean[:M], rstd[:M], dr, parts["dgamma"], parts["dbeta"], C + PAD, G, TORCH[c.g], c.p,
                                            rng, L.SITE, parts.get("gbias"), stream_dtype=TORCH[c.stream])
            assert g.dtype == TORCH[c.g] and g.shape == (M, C)
        assert dx.dtype == TORCH[c.stream] and dx.shape == (M, C)
        check_rows(c, "dx", dx, ref["dx"], mod["dx"], tol_dx, True)
        if g is not None:
            check_rows(c, "g", g, ref["g"], mod["g"], TOL_BWD[c.g], True)
            if keep is not None:
                dropped = keep[:M] == 0
                assert bool((g.cpu()[dropped] == 0).all()), f"{c.id} M={M}: a dropped element of g is not zero"
                assert M * C < 4096 or 0.15 < dropped.double().mean().item() < 0.25
        for n, t in sums:
            check_partials(c, n, parts[n], G, M, C, ref[t], ratios[n], dev)


@pytest.mark.parametrize("c", L.BWD_CASES, ids=lambda c: c.id)
def test_backward(dev, c):
    _backward_case(dev, c)


@pytest.mark.parametrize("c", L.FUSED_CASES, ids=lambda c: c.id)
def test_backward_fused(dev, c):
    _backward_case(dev, c)


@pytest.mark.parametrize("c", L.STREAM_CASES, ids=lambda c: c.id)
def test_backward_fused_bf16_stream(dev, c):
    """the prefetching instance: chunks of 1, 5, 9, 17, 18 and 33 rows against 16 / 8 waves with one or two rows in flight"""
    _backward_case(dev, c)


# ---------------------------------------------------------------------------------------------------------------------
# fp8 forms
# ---------------------------------------------------------------------------------------------------------------------
def _fp8_backward(dev, c, M, G, fp8_out_only=False):
    """one launch of the fused fp8 form and of the plain fused form on the same operands; returns what both left.
    fp8_out_only: the fp8 form does not write its bf16 g (the returned g is then uninitialised memory)"""
    ops = _ops()
    C, op = c.C, L.operands(c.C)
    ref, mod = L.backward_reference(C, c.dy, c.stream, c.dresid, c.p)
    x, w = op["x"][:M].to(dev), op["w"].to(dev)
    dy, dres = op["dy"][:M].to(TORCH[c.dy]).to(dev), op["dres"][:M].to(TORCH[c.stream]).to(dev)
    mean, rstd = _stats(C, dev)
    rng = ops.new_rng_state(L.SEED, dev, L.STEP)
    wr = L.STEP & 1                                                   # the slot the launch writes; the other one is read
    gmax = ref["g"][:M].abs().max().item()
    amax_prev = torch.tensor(0.8 * gmax, dtype=torch.float32)        # below this step's maximum: the cast clamps
    gen = torch.Generator().manual_seed(M + C)
    parts2 = torch.empty(2, G)
    parts2[wr ^ 1] = amax_prev * torch.rand(G, generator=gen)
    parts2[wr ^ 1, 9] = amax_prev
    parts2[wr] = float("nan")
    before = parts2.clone()
    parts2 = parts2.reshape(-1).to(dev)
    P0 = [_nan(dev, G, C + PAD) for _ in range(3)]
    P1 = [_nan(dev, G, C + PAD) for _ in range(3)]
    kw = dict(stream_dtype=TORCH[c.stream])
    dx0, g0 = ops.layernorm_bwd_fused(dy, x, w, mean[:M], rstd[:M], dres, P0[0], P0[1], C + PAD, G, torch.bfloat16, c.p, rng, L.SITE, P0[2], **kw)
    dx, g, g8, sinv = ops.layernorm_bwd_fused(dy, x, w, mean[:M], rstd[:M], dres, P1[0], P1[1], C + PAD, G, torch.bfloat16, c.p, rng, L.SITE, P1[2],
                                              fp8_out=(parts2, rng), fp8_out_only=fp8_out_only, **kw)
    torch.cuda.synchronize()
    return dict(ref=ref, mod=mod, dx0=dx0, g0=g0, P0=P0, dx=dx, g=g, g8=g8, sinv=sinv, P1=P1, parts2=parts2.cpu().view(2, G), before=before, wr=wr,
                amax_prev=amax_prev, gmax=gmax, keep=L.keep_scale(C, c.p)[:M])


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


@pytest.mark.parametrize("c,fp8_out_only", [pytest.param(c, only, id=c.id + ("-fp8_out_only" if only else ""))
                                            for only in (False, True) for c in L.FP8_BWD_CASES])
def test_backward_fused_fp8(dev, c, fp8_out_only):
    """n_partials = 256 at M = 100 / 300: 156 / 106 workgroups own no rows.  dx, g and the partial rows are what the call without
    fp8_out leaves, bit for bit; every entry of the history slot being written comes back finite, 0 for workgroups without rows,
    the slot's maximum is this step's max |g|; g8 is g at last step's scale within one e5m2 rounding, as
    tests/test_gpu_fp8.py::test_layernorm_bwd_fused_fp8_emits_the_next_gradient_operand has it at its sizes.
    fp8_out_only=True (the kernel's g8_only branch: the bf16 g is not written) leaves the same dx, g8, scale_inv, partial rows and
    history slot as the run that writes g, bit for bit."""
    C = c.C
    for M, G in c.rows:
        r = _fp8_backward(dev, c, M, G)
        if fp8_out_only:
            o = _fp8_backward(dev, c, M, G, fp8_out_only=True)
            for k in ("dx", "g8", "sinv"):
                assert torch.equal(_bits(o[k]), _bits(r[k])), f"{c.id} M={M}: {k} differs with fp8_out_only"
            assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(o["P1"], r["P1"])), f"{c.id} M={M}: a partial array differs with fp8_out_only"
            assert torch.equal(_bits(o["parts2"][o["wr"]]), _bits(r["parts2"][r["wr"]])), f"{c.id} M={M}: the written history slot differs with fp8_out_only"
            continue
        ref, mod, wr = r["ref"], r["mod"], r["wr"]
        assert torch.equal(_bits(r["dx"]), _bits(r["dx0"])) and torch.equal(_bits(r["g"]), _bits(r["g0"]))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(r["P0"], r["P1"]))
        check_rows(c, "dx", r["dx"], ref["dx"], mod["dx"], TOL_BWD[c.stream], True)
        check_rows(c, "g", r["g"], ref["g"], mod["g"], TOL_BWD[BF16], True)
        for i, (n, t) in enumerate((("dgamma", "dgamma_terms"), ("dbeta", "dbeta_terms"), ("gbias", "gbias_terms"))):
            check_partials(c, n, r["P1"][i], G, M, C, ref[t], column_ratio(mod[t], ref[t], [M]), dev)
        rows_per = -(-M // G)
        used = -(-M // rows_per)
        slot = r["parts2"][wr]
        assert bool(torch.isfinite(slot).all()), f"{c.id} M={M}: {int((~torch.isfinite(slot)).sum())} of {G} partial maxima were not written"
        assert bool((slot[used:] == 0).all()) and bool((slot[:used] > 0).all())
        assert abs(slot.max().item() - r["gmax"]) < 1e-5 * r["gmax"]
        assert torch.equal(_bits(r["parts2"][wr ^ 1]), _bits(r["before"][wr ^ 1]))                      # the slot that was read
        amax_prev = r["amax_prev"].item()
        assert abs(r["sinv"].item() - amax_prev / E5_MAX) < 1e-6 * amax_prev
        got = r["g8"].float().double().cpu() * r["sinv"].item()
        want = ref["g"][:M].clamp(min=-amax_prev, max=amax_prev)
        tol = want.abs() * (2.0 ** -3 + 1e-4) + amax_prev / E5_MAX * 2.0 ** -16 + 2e-6 * r["gmax"]
        assert bool(((got - want).abs() <= tol).all()) and bool((got[r["keep"] == 0] == 0).all())


@pytest.mark.parametrize("c", L.FP8_BWD_CASES, ids=lambda c: c.id)
def test_backward_fused_fp8_g8_is_the_cast_of_the_returned_g(dev, c):
    """g8 is the e5m2 cast of the RETURNED bf16 g at last step's scale, bit for bit: what dg_fp8_quantize_delayed makes of that g,
    so the fused form and the separate cast launch hand the next dX GEMM the same operand.  (Until this test the kernel cast
    the fp32 g before its bf16 rounding, and 0.5 - 0.9 % of the bytes at these sizes lay one e5m2 step away: 137 .. 2128 per case.)
    amax_prev lies below this step's maximum, so the clamp is reached."""
    seen = []
    for M, G in c.rows:
        r = _fp8_backward(dev, c, M, G)
        sc = (torch.tensor(E5_MAX) / r["amax_prev"]).to(dev)
        want = (r["g"].float() * sc).clamp(-E5_MAX, E5_MAX).to(E5)
        assert bool((want.float().abs() == E5_MAX).any()), "no element reaches the clamp"
        diff = _bits(r["g8"]) != _bits(want)
        seen.append((M, int(diff.sum()), diff.numel(), tuple(int(i) for i in diff.nonzero()[0]) if bool(diff.any()) else None))
        if os.environ.get("DG_TEST_REPORT"):
            print(f"[layernorm] {c.id} | g8 vs cast of bf16 g M={M} | {seen[-1][1]} of {seen[-1][2]} bytes differ ({seen[-1][1] / seen[-1][2]:.3%})", flush=True)
    assert all(n == 0 for _, n, _, _ in seen), f"{c.id}: bytes of g8 that differ from the e5m2 cast of the returned g (M, differ, of, first at): {seen}"


@pytest.mark.parametrize("c", L.FP8_FWD_CASES, ids=lambda c: c.id)
def test_forward_fp8(dev, c):
    """dg_layernorm_fwd_fp8 at M = 1, 7, 9, 100 (waves and, at M = 9, most of a workgroup without rows: they only feed the
    maxima): y, mean, rstd are dg_layernorm_fwd's bit for bit, the e4m3 bytes are the delayed cast of that y, the slot being
    written arrives as NaN and holds the output's maximum afterwards; y against fp64 as in test_forward."""
    ops = _ops()
    C, op = c.C, L.operands(c.C)
    ref, mod = L.forward_reference(C)
    x, w, b = op["x"].to(dev), op["w"].to(dev), op["b"].to(dev)
    for M in c.rows:
        n = ops.layernorm_fwd_fp8_parts(M)
        assert n == -(-M // 8)
        state = ops.new_rng_state(5, dev, 6)                          # step word 6: slot 0 is written, slot 1 read
        y0, mean0, rstd0 = ops.layernorm_fwd(x[:M], w, b, torch.bfloat16)
        amax_prev = torch.tensor(0.8 * ref["y"][:M].abs().max().item(), dtype=torch.float32)
        parts2 = torch.empty(2, n)
        parts2[1] = amax_prev * torch.rand(n, generator=torch.Generator().manual_seed(M))
        parts2[1, 7 % n] = amax_prev
        parts2[0] = float("nan")
        before = parts2.clone()
        parts2 = parts2.reshape(-1).to(dev)
        y, mean, rstd, q8, sinv = ops.layernorm_fwd_fp8(x[:M], w, b, parts2, state)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(y0)) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0)
        check_rows(c, "y", y, ref["y"], mod["y"], TOL_FWD[BF16], False)
        P.assert_layernorm_stats(mean, rstd, op["x"][:M], ref["mean"][:M], ref["std"][:M], ref["xhat"][:M], f"{c.id} M={M}")
        sc = torch.tensor(E4_MAX) / amax_prev
        assert abs(sinv.item() - 1.0 / sc.item()) < 1e-6 / sc.item()
        want = (y0.float() * sc.to(dev)).clamp(-E4_MAX, E4_MAX).to(torch.float8_e4m3fn)
        diff = _bits(q8) != _bits(want)
        assert not bool(diff.any()), f"{c.id} M={M}: {int(diff.sum())} e4m3 bytes differ from the cast of y, first at {tuple(int(i) for i in diff.nonzero()[0])}"
        after = parts2.cpu().view(2, n)
        assert torch.equal(after[1], before[1])                                        # the slot that was read
        assert bool(torch.isfinite(after[0]).all()), f"{c.id} M={M}: a partial maximum was not written"
        per_group = torch.nn.functional.pad(y0.float().abs().amax(1).cpu(), (0, 8 * n - M)).view(n, 8).amax(1)
        assert torch.equal(after[0], per_group), f"{c.id} M={M}: the partial maxima are not the 8-row groups' max |y|"
        y2, _, _, q8b, _ = ops.layernorm_fwd_fp8(x[:M], w, b, before.reshape(-1).to(dev), state, want_bf16=False)
        assert getattr(y2, "dg_unwritten", False) and torch.equal(_bits(q8b), _bits(q8))


# ---------------------------------------------------------------------------------------------------------------------
# rejections: an error code before any launch, every output untouched
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,C,mis,dy_t,g_t,stream_t", L.REJECTED,
                         ids=[f"{e}-C{C}-dy_{d}" + (f"-g_{g}" if g else "") + f"-stream_{s}" + (f"-{m}_plus4" if m else "") for e, C, m, d, g, s in L.REJECTED])
def test_rejected_before_any_launch(dev, entry, C, mis, dy_t, g_t, stream_t):
    """through the C ABI, with every output buffer (dx, g, the partial rows) owned by the test and filled with NaN beforehand"""
    from drakegpt_amd import _lib
    ops = _ops()
    assert L.instance(entry, C, mis is None, dy_t, g_t or F32, stream_t) == "rejected"
    M, G = 8, 4
    x, w = torch.zeros(M, C, device=dev), torch.ones(C, device=dev)
    mean, rstd = torch.zeros(M, device=dev), torch.ones(M, device=dev)
    dy = _put(torch.ones(M, C, dtype=TORCH[dy_t]), dev, mis == "dy")
    dx = _nan(dev, M, C, dtype=TORCH[stream_t])
    g = _put(torch.full((M, C), float("nan"), dtype=TORCH[g_t or F32]), dev, mis == "g")
    parts = [_nan(dev, G, C + PAD) for _ in range(3)]
    outs = [dx, g] + parts
    ptr = lambda t: t.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "bwd":
        rc = _lib.lib.dg_layernorm_bwd(ptr(dy), ops.dt_code(dy.dtype), ptr(x), ptr(w), ptr(mean), ptr(rstd), None, ptr(dx), ptr(parts[0]), ptr(parts[1]),
                                       C + PAD, G, M, C, stream)
    else:
        rc = _lib.lib.dg_layernorm_bwd_fused(ptr(dy), ops.dt_code(dy.dtype), ptr(x), ptr(w), ptr(mean), ptr(rstd), None, ptr(dx), ops.dt_code(dx.dtype),
                                             ptr(parts[0]), ptr(parts[1]), C + PAD, G, M, C, ptr(g), ops.dt_code(g.dtype), 0.0, None, 0, ptr(parts[2]), stream)
    torch.cuda.synchronize()
    assert rc != 0
    for t in outs:
        assert bool(torch.isnan(t).all()), "an output was written by a rejected call"


def test_rejections_through_ops_raise(dev):
    """the same through the tensor-level wrappers (which allocate dx and g themselves): RuntimeError, partial rows untouched"""
    ops = _ops()
    M, G = 8, 4
    for entry, C, mis, dy_t, g_t, stream_t in L.REJECTED:
        if mis == "g":
            continue                                         # (ops allocates g)
        x, w = torch.zeros(M, C, device=dev), torch.ones(C, device=dev)
        mean, rstd = torch.zeros(M, device=dev), torch.ones(M, device=dev)
        dy = _put(torch.ones(M, C, dtype=TORCH[dy_t]), dev, mis == "dy")
        pg, pb = _nan(dev, G, C), _nan(dev, G, C)
        with pytest.raises(RuntimeError):
            if entry == "bwd":
                ops.layernorm_bwd(dy, x, w, mean, rstd, None, pg, pb, C, G)
            else:
                ops.layernorm_bwd_fused(dy, x, w, mean, rstd, None, pg, pb, C, G, TORCH[g_t], 0.0, None, 0, None, stream_dtype=TORCH[stream_t])
        torch.cuda.synchronize()
        assert bool(torch.isnan(pg).all()) and bool(torch.isnan(pb).all()), (entry, C, mis)
