"""tests/layernorm_cases.py on the CPU: the restated dispatch names what csrc/layernorm.hip launches, the case tables of
tests/test_gpu_layernorm.py reach every template instance with all slices full and (where the width class allows) with a
partially filled last slice, and the fp32 model of oracle/parity.py, which sets the per-row bounds, stays inside the suite's
whole-tensor tolerances by itself.

INSTANCES is written out by hand from the launches of the kernel file (the two forward entry points and ln_bwd_launch, each over
the width table of ln_with_width), not derived from the tables: a new instance in the dispatch has to be added here, and then needs its cases."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layernorm_cases as L  # noqa: E402
from oracle import parity as P  # noqa: E402

F32, BF16 = L.F32, L.BF16

# (instance, "scalar" or the number of float4 slices per lane)
WIDTHS = ((1, 1024), (2, 1024), (3, 512), (4, 512), (8, 256))           # (LN_MAXV, backward threads) of the width table
INSTANCES = (
    # dg_layernorm_fwd: ln_fwd_scalar_kernel<TO> | ln_fwd_kernel<TO, 1 | 2 | 3 | 4 | 8>, TO = float | bf16_t
    [(f"ln_fwd_scalar_kernel<{o}>", "scalar") for o in (F32, BF16)]
    + [(f"ln_fwd_kernel<{o},{k}>", k) for o in (F32, BF16) for k, _ in WIDTHS]
    # dg_layernorm_fwd_fp8: ln_fwd_fp8_kernel<1 | 2 | 3 | 4>
    + [(f"ln_fwd_fp8_kernel<{k}>", k) for k, _ in WIDTHS[:4]]
    # ln_bwd_launch, fuse == 0: ln_bwd_scalar_kernel<1024 | 512 | 256>, ln_bwd_kernel<TD, K, NT, 0, float, 0> with dy float | bf16_t
    + [(f"ln_bwd_scalar_kernel<{nt}>", "scalar") for nt in (1024, 512, 256)]
    + [(f"ln_bwd_kernel<{d},{k},{nt},0,f32,0>", k) for d in (F32, BF16) for k, nt in WIDTHS]
    # fuse == 1 (bf16 g) and fuse == 2 (fp32 g): ln_bwd_kernel<TD, 1 .. 4, NT, F, float, 0> with dy float | bf16_t
    + [(f"ln_bwd_kernel<{d},{k},{nt},{f},f32,0>", k) for f in (1, 2) for d in (F32, BF16) for k, nt in WIDTHS[:4]]
    # the bf16 gradient stream: two rows in flight, one at LN_MAXV = 2
    + [(f"ln_bwd_kernel<bf16,{k},{nt},1,bf16,{1 if k == 2 else 2}>", k) for k, nt in WIDTHS[:4]]
)


def coverage_gaps(cases):
    """[(instance, what is missing)] of INSTANCES against a case list"""
    reached = {}
    for c in cases:
        reached.setdefault(c.instance, []).append(c)
    gaps = []
    for name, k in INSTANCES:
        mine = reached.get(name, [])
        kinds = [L.scalar_slices(c.C) if k == "scalar" else L.slices(c.C) for c in mine]
        if not any(full for full, _ in kinds):
            gaps.append((name, "no case with all slices full"))
        if not any(part for _, part in kinds):           # (every width class has ragged widths: nk = 1 below 256, LN_MAXV = 8 from 1028)
            gaps.append((name, "no case with a partially filled last slice"))
    return gaps


def test_instance_list_is_what_it_says():
    names = [n for n, _ in INSTANCES]
    assert len(set(names)) == len(names) == 12 + 4 + 13 + 16 + 4


def test_every_instance_has_a_full_and_a_ragged_case():
    assert coverage_gaps(L.ALL_CASES) == []
    assert "rejected" not in {c.instance for c in L.ALL_CASES}
    assert {c.instance for c in L.ALL_CASES} <= {n for n, _ in INSTANCES}, "a case reaches an instance that INSTANCES does not list"
    ids = [c.id for c in L.ALL_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("name", [n for n, _ in INSTANCES])
def test_the_coverage_check_notices_an_instance_without_cases(name):
    """delete the rows of one instance from the tables: the check above names it, for both kinds of case"""
    gaps = coverage_gaps([c for c in L.ALL_CASES if c.instance != name])
    assert sorted(gaps) == sorted([(name, "no case with all slices full"), (name, "no case with a partially filled last slice")])


def test_the_coverage_check_notices_missing_full_or_ragged_rows():
    """deleting ALL full (or all ragged) rows of an instance is noticed as well"""
    for name, k in INSTANCES:
        for want_full in (True, False):
            sl = L.scalar_slices if k == "scalar" else L.slices
            kept = [c for c in L.ALL_CASES if not (c.instance == name and sl(c.C)[0 if want_full else 1])]
            assert any(g[0] == name for g in coverage_gaps(kept)), (name, want_full)


# The ids of test_the_restated_dispatch, one per case below: a case keeps the id it had while the scalar kernels were still the
# VEC = false instances of ln_fwd_kernel / ln_bwd_kernel and the prefetching ones were spelled "pipe", so that a case is one test
# over the project's history.  The expected strings are the current spelling.
DISPATCH_IDS = [
    "args0-ln_fwd_kernel<f32,true,2>",
    "args1-ln_fwd_kernel<f32,false,1>",
    "args2-ln_fwd_kernel<f32,false,1>",
    "args3-ln_fwd_kernel<f32,true,8>",
    "args4-ln_fwd_kernel<f32,true,8>",
    "args5-ln_fwd_kernel<f32,true,1>",
    "args6-ln_fwd_kernel<f32,false,1>",
    "args7-ln_fwd_fp8_kernel<1>",
    "args8-ln_fwd_fp8_kernel<2>",
    "args9-rejected",
    "args10-rejected",
    "args11-ln_bwd_kernel<f32,true,2,1024,0>",
    "args12-ln_bwd_kernel<bf16,true,2,1024,0>",
    "args13-ln_bwd_kernel<f32,false,1,1024,0>",
    "args14-ln_bwd_kernel<f32,false,1,512,0>",
    "args15-ln_bwd_kernel<f32,false,1,256,0>",
    "args16-ln_bwd_kernel<f32,true,8,256,0>",
    "args17-ln_bwd_kernel<f32,true,4,512,0>",
    "args18-ln_bwd_kernel<f32,true,3,512,0>",
    "args19-ln_bwd_kernel<bf16,true,2,1024,1>",
    "args20-ln_bwd_kernel<f32,true,4,512,2>",
    "args21-ln_bwd_kernel<bf16,true,2,1024,1,bf16,pipe>",
    "args22-ln_bwd_kernel<bf16,true,4,512,1,bf16,pipe>",
    "args23-ln_bwd_kernel<bf16,true,2,1024,1,bf16,pipe>",
    "args24-rejected",
]


@pytest.mark.parametrize("args,want", [
    (("fwd", 384), "ln_fwd_kernel<f32,2>"), (("fwd", 384, False), "ln_fwd_scalar_kernel<f32>"), (("fwd", 4096), "ln_fwd_scalar_kernel<f32>"),
    (("fwd", 2048), "ln_fwd_kernel<f32,8>"), (("fwd", 1028), "ln_fwd_kernel<f32,8>"), (("fwd", 4), "ln_fwd_kernel<f32,1>"),
    (("fwd", 3), "ln_fwd_scalar_kernel<f32>"), (("fwd_fp8", 256), "ln_fwd_fp8_kernel<1>"), (("fwd_fp8", 260), "ln_fwd_fp8_kernel<2>"),
    (("fwd_fp8", 1028), "rejected"), (("fwd_fp8", 30), "rejected"),
    (("bwd", 384), "ln_bwd_kernel<f32,2,1024,0,f32,0>"), (("bwd", 384, True, BF16), "ln_bwd_kernel<bf16,2,1024,0,f32,0>"),
    (("bwd", 510), "ln_bwd_scalar_kernel<1024>"), (("bwd", 1001), "ln_bwd_scalar_kernel<512>"),
    (("bwd", 2046), "ln_bwd_scalar_kernel<256>"), (("bwd", 2048), "ln_bwd_kernel<f32,8,256,0,f32,0>"),
    (("bwd", 772), "ln_bwd_kernel<f32,4,512,0,f32,0>"), (("bwd", 516), "ln_bwd_kernel<f32,3,512,0,f32,0>"),
    (("bwd_fused", 384, True, BF16, BF16), "ln_bwd_kernel<bf16,2,1024,1,f32,0>"), (("bwd_fused", 1024, True, F32, F32), "ln_bwd_kernel<f32,4,512,2,f32,0>"),
    (("bwd_fused", 384, True, BF16, BF16, BF16), "ln_bwd_kernel<bf16,2,1024,1,bf16,1>"),
    (("bwd_fused", 1024, True, BF16, BF16, BF16), "ln_bwd_kernel<bf16,4,512,1,bf16,2>"),
    (("bwd_fused_fp8", 384, True, BF16, BF16, BF16), "ln_bwd_kernel<bf16,2,1024,1,bf16,1>"),
    (("bwd_fused", 384, True, BF16, F32, F32, True), "rejected"),
], ids=DISPATCH_IDS)
def test_the_restated_dispatch(args, want):
    assert L.instance(*args) == want


def test_the_rejections_are_rejections_and_the_last_accepted_width_is_not():
    for entry, C, mis, dy, g, stream in L.REJECTED:
        assert L.instance(entry, C, mis is None, dy, g or F32, stream) == "rejected", (entry, C, mis, dy, g, stream)
    assert L.instance("bwd", 2046) != "rejected" and 2 * 4 * 2046 * 4 <= 65536 < 2 * 4 * 2050 * 4
    # the 64 KB rule of the unfused form bites only beyond the widths the vector path serves
    assert all(L.instance("bwd", C) != "rejected" for C in range(1, 2049))
    assert all(L.instance("bwd", C) == "rejected" for C in (2049, 2050, 4096))
    from drakegpt_amd.ops import layernorm_bwd_fused_supported      # (imports without the library's GPU: host logic only)
    for C in (4, 30, 100, 1024, 1028, 2048):
        assert layernorm_bwd_fused_supported(C) == (L.instance("bwd_fused", C) != "rejected"), C


def test_the_row_sets_reach_what_they_are_chosen_for():
    empty = lambda M, G: G - -(-M // -(-M // G))             # workgroups of G whose chunk starts at or beyond M
    assert [empty(M, G) for M, G in L.ROWS_BWD] == [3, 19, 2, 0, 0]
    for nw in (16, 8, 4):
        per = [-(-M // G) for M, G in L.ROWS_BWD]
        assert min(per) < nw and max(per) > 2 * nw                      # fewer rows than waves; more than two rounds per wave
    assert [empty(M, G) for M, G in L.ROWS_FP8_BWD] == [156, 106]
    # the prefetching instance (PD rows in flight, PD = 1 at nk = 2, else 2): chunks shorter than, equal to and one beyond
    # NW, 2 NW (+ 1) for NW = 16 (C <= 512) and NW = 8
    per = [-(-M // G) for M, G in L.ROWS_STREAM]
    assert per == [1, 5, 9, 17, 18, 33]
    assert any(M % 8 for M in L.ROWS_FWD) and min(L.ROWS_FWD) == 1 and 9 in L.ROWS_FWD and any(M % 8 and M < 8 for M in L.ROWS_FP8_FWD)


# ---------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 100, 384])
def test_model_formulas_in_fp64_are_autograd(C):
    """layernorm_model evaluated in double is the reference: its dx, y and column-sum terms equal autograd's"""
    ref, _ = L.backward_reference(C, F32, F32, True, 0.2)
    op = L.operands(C)
    m = P.layernorm_model(op["x"], op["w"], op["b"], op["dy"], op["dres"], L.keep_scale(C, 0.2), 0.2, dtype=torch.float64)
    fwd = L.forward_reference(C)[0]
    assert P.rel(m["y"], fwd["y"]) < 1e-14 and P.rel(m["rstd"], fwd["rstd"]) < 1e-14
    for k in ("dx", "g", "dgamma_terms", "dbeta_terms", "gbias_terms"):
        assert P.rowwise_rel(m[k], ref[k], C).max().item() < 1e-11, k          # (C = 3: dx cancels to ~1e-3 of its terms)
    xd, wd, bd = (op[k].double().requires_grad_(True) for k in ("x", "w", "b"))
    torch.nn.functional.layer_norm(xd, (C,), wd, bd, 1e-5).backward(op["dy"].double())
    assert P.rel(ref["dgamma_terms"].sum(0), wd.grad) < 1e-13 and P.rel(ref["dbeta_terms"].sum(0), bd.grad) < 1e-13


MODEL_WIDTHS = sorted(set(C for C in L.SCALAR_WIDTHS + L.VECTOR_WIDTHS + L.STREAM_WIDTHS + (4096,) if C >= 32))


@pytest.mark.parametrize("C", MODEL_WIDTHS)
def test_model_alone_stays_inside_the_whole_tensor_tolerances(C):
    """the fp32 model at the seeds of the cases: forward 1e-6 (4e-3 once rounded to bf16), backward 2e-6, column sums 3e-6 --
    the tolerances of tests/test_gpu_ops.py that the GPU tests keep as their first assertion at C >= 32"""
    ref, mod = L.forward_reference(C)
    assert P.rel(mod["y"], ref["y"]) < 1e-6 and P.rel(P.rb(mod["y"]), ref["y"]) < 4e-3
    if C > 2048:
        return
    for dy in (F32, BF16):
        for dresid, p in ((True, 0.2), (False, 0.0)):
            ref, mod = L.backward_reference(C, dy, F32, dresid, p)
            assert P.rel(mod["dx"], ref["dx"]) < 2e-6 and P.rel(mod["g"], ref["g"]) < 2e-6
            assert P.rel(P.rb(mod["g"]), ref["g"]) < 3e-3
            for k in ("dgamma_terms", "dbeta_terms", "gbias_terms"):
                for M in (1, 40, 517):
                    assert P.rel(mod[k][:M].sum(0), ref[k][:M].sum(0)) < 3e-6, (k, M)
