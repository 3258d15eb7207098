"""The table of dg_gemm_nt calls that tests/test_gpu_nt_instances.py runs (tests/nt_run_cases.py), on the CPU: every kernel the
library can launch is planned by a case, every case is what it is named for (by the library's own plan of made-up addresses with
the views' alignment, at 256 CUs -- and, for everything but the fp8-copy forms, at 304 and 64), every class of K-step count, tile
kind, ragged edge and layout flip is covered for every operand family, and the operands meet the conditions the GPU test's
claims rest on: exact data stays exactly representable, the undecided share of the sign decisions stays small, the split
contraction's emulation stays inside its derived envelope."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nt_cases as T  # noqa: E402
import nt_run_cases as R  # noqa: E402
from oracle import parity as P  # noqa: E402
from test_nt_cases_host import STAGED, listed_instances  # noqa: E402

CASES = R.run_cases(256)
WS = [c for c in CASES if c.ws]
FAMILIES = (R.BF16, R.E4M3, R.E5M2, R.X3)
SMALL = [c for c in CASES if c.M * c.N <= 256 * 201]


def plan(case, ncu=256):
    return T.plan_of(R.host_args(case, ncu), ncu, 0)


def test_every_kernel_is_planned_and_every_case_is_what_it_is_named_for():
    every = set().union(*listed_instances().values())
    assert len(every) == 74 and len(STAGED) == 4 and set(R.STAGED.values()) == STAGED
    got = set()
    for c in CASES:
        pl = plan(c)
        R.check_plan(c, pl, 256)
        got.add(pl.name)
    assert got == every | STAGED, ((every | STAGED) - got, got - every - STAGED)
    assert [c.name for c in CASES] == R.CASE_NAMES and len(set(R.CASE_NAMES)) == len(CASES)
    # the CU count enters the uneven shapes alone; the fp8 copy exists on exactly 256 CUs
    for ncu in (304, 64):
        scaled = R.run_cases(ncu)
        assert [c.name for c in scaled] == R.CASE_NAMES
        for c, c256 in zip(scaled, CASES):
            assert c.uneven or c == c256
            if "fp8_out" in c.opts:
                assert plan(c, ncu).rc == -1
            else:
                R.check_plan(c, plan(c, ncu), ncu)


def test_flags_both_ways():
    plans = [(c, plan(c)) for c in CASES]
    for f in ("vec_ok", "mask_vec_ok", "drop", "warm_b"):
        assert {bool(getattr(pl, f)) for c, pl in plans if c.ws} == {False, True}, f
    assert {pl.cs_accum for c, pl in plans if "colsum" in c.opts} == {0, 1}
    assert {(c.uneven, pl.cs_accum) for c, pl in plans if "colsum" in c.opts} >= {(True, 1), (True, 0), (False, 1), (False, 0)}
    for c, pl in plans:                                               # a flip is a flip: the plan's flag follows the view
        if c.flip("c_off") or c.flip("ldr") % 4 or c.flip("res_off") or c.flip("ldc", c.N) % 4:
            assert pl.vec_ok == 0, c.name
        if c.flip("ldmask") % 4 or c.flip("mask_off"):
            assert pl.mask_vec_ok == 0, c.name
    # the un-prefetched reader of the sign bits: a misaligned bias, C or row pitch under a sign_bits input
    unpf = [c for c, pl in plans if "sign_bits" in c.opts and pl.pf == 0 and c.ws]
    assert {c.ind for c in unpf} == {R.BF16, R.E4M3, R.E5M2} and any(c.flip("bias_off") for c in unpf) and any(c.flip("c_off") for c in unpf)


@pytest.mark.parametrize("ind", FAMILIES)
def test_classes_per_family(ind):
    fam = [c for c in WS if c.ind == ind]
    base = 2 * R.KSTEP[ind] if ind != R.X3 else 128
    assert {c.nk for c in fam} >= ({4, 5, 9} if ind == R.X3 else set(R.NK))
    assert {c.K for c in fam} >= {R.BF16: {128, 192, 256, 320, 576}, R.X3: {128, 160, 288}}.get(ind, {256, 384, 512, 640, 1152})
    assert {c.N % 192 == 0 for c in fam} == {False, True}
    has = lambda pred: any(pred(c) for c in fam)
    assert has(lambda c: c.M == 200 and c.N == 192) and has(lambda c: c.M == 200 and c.N % 192)       # ragged M, both widths
    assert has(lambda c: c.N == 200) and has(lambda c: c.M == 200 and c.N == 200)                     # ragged N, N % 8 == 0
    assert has(lambda c: c.N == 100 and c.flip("ldc", c.N) % 4 == 0)
    assert has(lambda c: (c.N, c.flip("ldc", c.N)) == (201, 204) and "drop" in c.opts)
    assert has(lambda c: (c.N, c.flip("ldc", c.N)) == (99, 99) and "drop" in c.opts)
    assert has(lambda c: c.uneven) and has(lambda c: not c.uneven)
    assert all(c.K == base for c in fam if c.uneven)                  # "K of two steps" (the split form's floor: four)
    for key in ("lda", "ldb", "ldc", "c_off", "ldr", "res_off", "bias_off"):
        assert has(lambda c: c.flip(key)), key
    if ind in (R.BF16, R.X3):
        assert has(lambda c: c.flip("ldmask")) and has(lambda c: c.flip("mask_off"))
    if ind in (R.BF16, R.E5M2):                                       # the mask prefetch at every K-step count (pf_at = nk - 3, floor 0)
        assert {c.nk for c in fam if ",true," in c.kernel} >= set(R.NK)
    if ind in (R.E4M3, R.E5M2):
        big = {(c.M, c.N, "fp8_out_only" in c.opts) for c in fam if "fp8_out" in c.opts}
        assert {(8192, 512), (4096, 1536)} <= {b[:2] for b in big} and {b[2] for b in big} == {False, True}


def test_staged_kernels():
    for (ind, outd), name in R.STAGED.items():
        mine = [c for c in CASES if c.kernel == name]
        assert {c.K for c in mine} >= {8, 40, 104 if ind == R.BF16 else 100}, name
        assert any("drop" in c.opts and c.N % 2 for c in mine) and any("relu_mask" in c.opts for c in mine), name
        assert all(plan(c).grid == plan(c).n_tiles and plan(c).block == 256 for c in mine)


def test_shapes_stay_small():
    """the largest are the uneven cases and the four fp8-copy shapes"""
    for c in CASES:
        if c.uneven:
            assert c.M * c.N <= 16640 * 384 and c.nk == (4 if c.ind == R.X3 else 2), c.name
        elif "fp8_out" in c.opts:
            assert c.M * c.N <= 4096 * 1536 and c.K == 256, c.name
        else:
            assert c.M <= 1024 and c.N <= 201 and c.K <= 1152, c.name


@pytest.mark.parametrize("name", [c.name for c in SMALL])
def test_conditions_on_the_operands(name):
    """on the reference alone: exactness of the exact run; the undecided share and the split emulation of the randn run.  (The
    large shapes are drawn from the same distributions; their conditions are asserted where they run.)"""
    case = CASES[R.CASE_NAMES.index(name)]
    sign = R.mask_operands(case.M, case.N)[3] if "sign_bits" in case.opts else None
    d = R.operands(case, "exact")
    r = R.reference(case, d, sign)
    assert R.exact_conditions(case, d, r) < 2 ** 24
    if "relu_mask" in d:
        m = d["relu_mask"].float()
        assert bool((m == 0).any()) and bool(torch.signbit(m[m == 0]).any()) and bool((~torch.signbit(m[m == 0])).any())
    if sign is not None:
        assert 0.2 < sign.double().mean().item() < 0.8
    d = R.operands(case, "randn")
    r = R.reference(case, d, sign)
    env, pre_env = R.envelopes(case, d, r)
    if "relu" in case.opts or "sign_bits_out" in case.opts:
        P.mask_margin(r["pre"], pre_env)                              # asserts its own max_share
    if case.ind == R.X3:
        A, B = d["A"], d["B"]
        err = (P.x3_emulation(A, B) - A.double() @ B.double().T).abs()
        bound = P.x3_envelope(A, B, case.K)
        assert bool((err <= bound).all()), (name, (err / bound).max().item())
        assert (err / bound).max().item() > 1e-3                      # ... and the envelope is of the error's own order


def test_x3_envelope_constant():
    """the split's worst case: x = 1 + 2^-8 is a bf16 tie, hi = 1 and lo = 2^-8 -- twice 2^-9 |x|; and a product of two such values
    against its three-term emulation uses the per-product bound 3 u^2 (1 + u) to a third (one of its three terms, at full size)"""
    x = torch.tensor([[1.0 + 2.0 ** -8]])
    hi, lo = P.split_bf16(x)
    assert hi.item() == 1.0 and lo.item() == 2.0 ** -8 > 2.0 ** -9 * x.item()
    err = abs(P.x3_emulation(x, x).item() - x.double().item() ** 2)
    assert err == 2.0 ** -16 and err <= P.X3_SPLIT * x.item() ** 2 < 3.1 * err
    assert P.x3_envelope(x, x, 1).item() == (P.X3_SPLIT + 3 * 2.0 ** -24) * x.double().item() ** 2


def test_epilogue_reference_order():
    """P.gemm_nt_epilogue_fp64 on one element per rule: the residual is added behind the dropout, the masks act behind the ReLU, the
    emitted bit is that of the final value, -0.0 in the tensor mask drops"""
    one = lambda **kw: P.gemm_nt_epilogue_fp64(torch.tensor([[3.0]]), **kw)
    t = lambda v: torch.tensor([[float(v)]])
    assert one(bias=t(-5), relu=True, residual=t(2))["out"].item() == 2.0
    assert one(bias=t(1), keep=t(1), p=0.5, residual=t(1))["out"].item() == 9.0
    assert one(keep=t(0), p=0.5, residual=t(-1))["bit"].item() is False
    assert one(relu_mask=t(-0.0))["out"].item() == 0.0 and one(relu_mask=t(0.5))["out"].item() == 3.0
    assert one(sign_mask=t(0), bias=t(4))["out"].item() == 0.0 and one(sign_mask=t(0), bias=t(4))["pre"].item() == 7.0
    r = P.gemm_nt_epilogue_fp64(torch.tensor([[1.0, -2.0], [3.0, 4.0]]))
    assert r["colsum"].tolist() == [4.0, 2.0] and r["bit"].tolist() == [[True, False], [True, True]]
