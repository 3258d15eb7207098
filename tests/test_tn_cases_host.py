"""tests/tn_cases.py on the CPU, and the host side of the dW (TN) GEMMs of csrc/gemm.hip: the kernel names the library's launch
plan can return are the hipLaunchKernelGGL targets of the TN launch sites (read from the source text), the port of tn_work is
a bijection onto (tile, split), CASES(ncu) reaches every class it lists for three CU counts, and the split-K workspace of a
grouped call holds every launch of the call: the reported size covers each launch, and no launch's hand-over flags lie where a
launch of the same call keeps partials.  The two layouts that showed the two defects of that path are named regression cases."""
import os
import random
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tn_cases as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "drakegpt_amd", "csrc", "gemm.hip")
NCUS = (256, 304, 64)


def launch_targets():
    text = open(SOURCE).read()
    return set(re.findall(r"hipLaunchKernelGGL\(\(?(gemm_tn_\w+)", text))


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_kernel_names_are_the_launch_targets():
    targets = launch_targets()
    assert targets == {"gemm_tn_ws_kernel", "gemm_tn_bf16_kernel", "gemm_tn_f32_kernel", "gemm_tn_x3_kernel", "gemm_tn_grouped256_kernel"}
    names = set()
    for dtype in (T.BF16, T.F32, T.X3):
        for R, Pn, Q, S in ((64, 128, 128, 1), (100, 128, 128, 1), (1024, 768, 768, 8), (64, 2048, 2048, 2)):
            names.add(T.plan(R, Pn, Q, S, dtype, 256).kernel)
    assert names == targets - {"gemm_tn_grouped256_kernel"}
    # the launch sites take their kernel from the plan: one launch per name, inside dg_gemm_tn's switch
    text = open(SOURCE).read()
    body = text[text.index('extern "C" int dg_gemm_tn('):text.index('extern "C" int dg_debug_tn_plan(')]
    assert "tn_plan(" in body and sorted(re.findall(r"hipLaunchKernelGGL\((gemm_tn_\w+)", body)) == sorted(names)
    launch = text[text.index("static int tn_grouped_launch("):text.index('extern "C" int dg_gemm_tn_grouped(')]
    assert launch.count("tn_grouped_plan(") == 2 and launch.count("hipLaunchKernelGGL") == 1


def test_plan_values():
    p = T.plan(1024, 384, 384, 7, T.BF16, 256)
    assert p == T.Plan("gemm_tn_ws_kernel", 0, 9, 7, 768, 192, 3, 9)
    p = T.plan(1000, 384, 128, 4, T.F32, 256)
    assert p == T.Plan("gemm_tn_f32_kernel", 1, 16, 1, 256, 256, 1, 3)            # share 2: ceil(3 / 2) * 8 workgroups, one of them padding
    p = T.plan(1024, 384, 128, 16, T.X3, 256)
    assert p == T.Plan("gemm_tn_x3_kernel", 1, 48, 1, 256, 64, 1, 3)
    assert T.plan(1024, 768, 768, 8, T.BF16, 256).kernel == "gemm_tn_bf16_kernel"          # 288 workgroups: two rounds
    assert T.plan(1024, 768, 768, 7, T.BF16, 256).kernel == "gemm_tn_ws_kernel"
    assert T.plan(1024, 768, 768, 8, T.BF16, 304).kernel == "gemm_tn_ws_kernel"
    assert T.plan(64, 128, 128, 1, T.BF16, 0).kernel == "gemm_tn_ws_kernel"                # 0: the device's count, 256 without one


@pytest.mark.parametrize("S", range(1, 33))
def test_tn_work_is_a_bijection(S):
    for n in range(1, 41):
        p = T.plan(64 * S, 128 * n, 128, S, T.BF16, 256)
        assert p.n_tiles == n
        seen = {}
        for by in range(p.grid_y):
            for bx in range(p.grid_x):
                tile, split = T.tn_work(bx, by, n, S, p.xcd_map)
                assert tile >= 0 and 0 <= split < S, (S, n, bx, by)
                if tile < n:
                    assert (tile, split) not in seen, (S, n, bx, by, seen[(tile, split)])
                    seen[(tile, split)] = (bx, by)
        assert len(seen) == n * S, (S, n)
        if p.xcd_map:                                       # every tile of a split on the split's own XCDs (id % 8)
            xcds = {}
            for (tile, split), (bx, _) in seen.items():
                xcds.setdefault(split, set()).add(bx % 8)
            share = max(8 // S, 1)
            assert all(len(x) <= share for x in xcds.values()), (S, n, xcds)


def test_xcd_remap_is_a_permutation():
    for n in list(range(1, 70)) + [162, 270]:
        assert sorted(T.xcd_remap(i, n) for i in range(n)) == list(range(n))


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncu", NCUS)
def test_cases_reach_every_class(ncu):
    mats, groups = T.CASES(ncu)
    assert len({c.name for c in mats}) == len(mats) and len({c.name for c in groups}) == len(groups)
    got = [c.check_class(ncu) for c in mats]                 # each case is the case it is named for
    assert {(k, m) for k, m, _ in got} == T.MAT_CLASSES
    assert T.NK_CLASSES <= {(k, nk) for k, _, nk in got}, T.NK_CLASSES - {(k, nk) for k, _, nk in got}
    by = {c.name: c for c in mats}
    # the staged bf16 kernel by both routes: a ragged R, and whole steps in more than one round of workgroups
    two = by["two-rounds"]
    pl = T.plan(two.R, two.P, two.Q, two.S, T.BF16, ncu)
    assert two.R % 64 == 0 and pl.n_tiles * two.S > ncu >= pl.n_tiles * (two.S - 1) and pl.kernel == "gemm_tn_bf16_kernel"
    assert by["bf16-1-ragged-steps"].R % 64 and T.plan(40, 128, 128, 1, T.BF16, ncu).kernel == "gemm_tn_bf16_kernel"
    # a tile count that is no multiple of the share, i.e. padding workgroups, at S = 1, 2, 4
    for S in (1, 2, 4):
        c = by[f"ws-map-S{S}"]
        pl = T.plan(c.R, c.P, c.Q, S, T.BF16, ncu)
        assert pl.n_tiles % (8 // S) and pl.grid_x * pl.grid_y > pl.n_tiles * S
    # every edge shape in every layout it admits, on every kernel
    edges = {(c.kind, c.P, c.Q, c.layout) for c in mats if c.layout != "plain"}
    assert edges == {(k, Pn, Q, lay) for k in T.KINDS for Pn, Q in T.EDGE_SHAPES for lay in ("padded", "out+1") + (("ldo4",) if Q % 4 else ())}
    for c in mats:
        lay = T.layout(c)
        if c.layout == "padded":
            assert lay.lda > T._ru(c.P, T.CHUNK[c.dtype]) and lay.ldo == c.Q + 5 and lay.stride == lay.slab + 37
        if c.layout == "ldo4":
            assert lay.ldo % 4 == 0 and c.Q % 4 and lay.ldo > c.Q
    # the empty last split of the ws kernel: the slab that must come out as zeros
    e = by["ws-empty-last-split"]
    assert T.slab_rows(e.R, e.S, T.plan(e.R, e.P, e.Q, e.S, T.BF16, ncu).r_per_split) == [(0, 64), (64, 128), (128, 128)]
    # grouped
    for g in groups:
        g.check_class(ncu)
    classes = {g.group_class(ncu) for g in groups}
    assert T.GROUP_CLASSES <= classes, T.GROUP_CLASSES - classes
    for body in T.MULTI_BODIES:
        assert any(b == body and n == "multi" and 2 in modes for b, n, modes in classes), (body, classes)
    halves = {(g.R // 128) for g in groups if g.f8 and len(g.shapes) == 1}
    assert halves == {1, 2, 3, 4}                            # one K step (never cut), halves of 1 + 1, 1 + 2, 2 + 2


def test_the_coverage_check_notices_a_missing_case():
    mats, _ = T.CASES(256)
    for drop in ("x3-map-S16", "f32-map-S8", "bf16-map-S4", "ws-map-S4"):
        got = {c.check_class(256)[:2] for c in mats if c.name != drop}
        assert T.MAT_CLASSES - got, drop
    got = {(k, nk) for k, _, nk in (c.check_class(256) for c in mats if c.name != "ws-3-steps")}
    assert T.NK_CLASSES - got == {("ws", (3, "full", False))}


# ---------------------------------------------------------------------------------------------------------------------
# the split-K workspace of a grouped call
# ---------------------------------------------------------------------------------------------------------------------
def check_workspace(shapes, f8, ncu):
    """this test's own arithmetic on the reported launches: partials of tile t at t * 128 KB, 8 flag words per tile from
    flag_offset, the error word in the last 16 bytes of the reported size"""
    launches = T.grouped_plan(shapes, f8, True, ncu)
    reported = T.workspace_bytes(shapes)
    step = T.MAX_GROUP[f8]
    assert [(l.first, l.count) for l in launches] == [(b, min(step, len(shapes) - b)) for b in range(0, len(shapes), step)]
    for l in launches:
        assert l.tiles == sum(T.group_tiles(Pn, Q) for _, Pn, Q in shapes[l.first:l.first + l.count])
    cut = [l for l in launches if l.splits != 1]
    for l in cut:
        assert l.ws_need <= reported, (l, reported)
        assert l.tiles * T.PART_BYTES <= reported - 16 and l.flag_offset + 32 * l.tiles <= reported - 16, (l, reported)
        assert l.flag_offset % 16 == 0
        for m in cut:                                        # m's partials: [0, m.tiles * 128 KB)
            assert l.flag_offset >= m.tiles * T.PART_BYTES, (l, m)
    assert all(l.ws_need == 0 for l in launches if l.splits == 1)
    return launches, reported


@pytest.mark.parametrize("ncu", NCUS)
@pytest.mark.parametrize("f8", [False, True])
def test_workspace_holds_every_launch_of_random_calls(f8, ncu):
    rnd = random.Random(1000 * ncu + f8)
    n_cut = 0
    for _ in range(300):
        n = rnd.randint(1, 130)
        kr = 128 if f8 else 64
        heavy = rnd.random() < 0.3                           # a stretch of larger problems somewhere in the list
        lo = rnd.randint(0, n)
        shapes = []
        for i in range(n):
            t = rnd.choice((1, 1, 1, 2, 3)) if not (heavy and lo <= i < lo + 40) else rnd.choice((2, 4, 6, 12))
            tp = rnd.choice([d for d in (1, 2, 3, 4, 6, 12) if t % d == 0])
            shapes.append((kr * rnd.randint(2, 5), 256 * tp - rnd.randint(0, 255), 128 * (t // tp) - rnd.randint(0, 127)))
        launches, _ = check_workspace(shapes, f8, ncu)
        n_cut += sum(l.splits != 1 for l in launches)
    assert n_cut > 100                                       # the property was exercised


@pytest.mark.parametrize("f8", [False, True])
def test_workspace_size_covers_both_chunkings(f8):
    """the size function has no dtype argument: one number must serve a call made with either operand kind"""
    one, two = (256, 128, 128), (256, 512, 128)
    shapes = [one] * 48 + [two] * 48 + [one] * 4
    assert T.workspace_bytes(shapes) == 96 * (T.PART_BYTES + 32) + 16           # the fp8 chunking's second launch (windows of 64: 80 tiles)
    shapes = [one] * 64 + [two] * 64 + [one] * 2
    assert T.workspace_bytes(shapes) == 128 * (T.PART_BYTES + 32) + 16          # the bf16 chunking's second launch (windows of 48: 96 tiles)
    check_workspace(shapes, f8, 256)


def test_regression_flags_of_a_small_launch_inside_the_partials_of_a_large_one():
    """70 one-tile bf16 problems at R = 128 on 256 CUs: launches of 64 and 6 tiles, both cut.  With the flags behind each launch's
    OWN partials, those of the second launch lay at 6 * 128 KB: in the first launch's partials of tile 6."""
    case = {g.name: g for g in T.group_cases(256)}["bf16-70x1"]
    launches, reported = check_workspace(case.rpq, False, 256)
    assert [(l.tiles, l.splits) for l in launches] == [(64, 2), (6, 2)]
    assert {l.flag_offset for l in launches} == {64 * T.PART_BYTES} and reported == 64 * (T.PART_BYTES + 32) + 16
    # the second form: the larger launch comes second and its partials covered the first launch's flags
    case = {g.name: g for g in T.group_cases(256)}["bf16-64x1+8x12"]
    launches, reported = check_workspace(case.rpq, False, 256)
    assert [(l.tiles, l.splits) for l in launches] == [(64, 2), (96, 2)]
    # (behind the largest launch under EITHER chunking: problems 48 .. 71 are 16 + 8 x 12 = 112 tiles)
    assert {l.flag_offset for l in launches} == {112 * T.PART_BYTES}


def test_regression_fp8_launch_larger_than_any_window_of_64():
    """48 one-tile, 48 two-tile and 4 one-tile fp8 problems: no window of 64 problems holds more than 80 tiles, the second fp8
    launch has 96 and is cut.  Sized by windows of 64 alone the workspace ended 2 MB before that launch's partials did."""
    case = {g.name: g for g in T.group_cases(256)}["fp8-48x1+48x2+4x1"]
    tiles = [T.group_tiles(Pn, Q) for Pn, Q in case.shapes]
    assert max(sum(tiles[b:b + 64]) for b in range(0, 100, 64)) == 80
    launches, reported = check_workspace(case.rpq, True, 256)
    assert [(l.tiles, l.splits) for l in launches] == [(48, 2), (96, 2), (4, 2)]
    assert reported == 96 * (T.PART_BYTES + 32) + 16 and reported - 80 * (T.PART_BYTES + 32) - 16 > 2 * 1000 * 1000


def test_grouped_launch_refuses_a_short_workspace_before_launching():
    """dg_gemm_tn_grouped returns DG_ERR_ARG (-1) for a workspace one byte short; nothing is enqueued (no GPU is needed to see the
    refusal: the size check comes before any launch)"""
    import ctypes as C
    L = T._lib()
    case = {g.name: g for g in T.group_cases(256)}["fp8-48x1+48x2+4x1"]
    arr = T.problem_array(case.rpq)
    buf = (C.c_char * 64)()
    addr = (C.addressof(buf) + 15) // 16 * 16
    for t in arr:                                            # (never dereferenced: the call is refused on its sizes)
        t.A = t.B = t.out = t.scale_a = t.scale_b = addr
        t.lda, t.ldb, t.ldo = 512, 256, 256
    need = T.workspace_bytes(case.rpq)
    assert L.lib.dg_gemm_tn_grouped(arr, len(arr), T.FP8_CODE, addr, need - 1, None) == -1
    assert L.lib.dg_gemm_tn_grouped(arr, len(arr), T.FP8_CODE, addr, 80 * (T.PART_BYTES + 32) + 16, None) == -1


# ---------------------------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------------------------
def test_exact_operands_stay_exact():
    import torch
    mats, groups = T.CASES(256)
    for c in mats:
        assert c.R * 16 < 2 ** 24                            # every partial sum of integers in [-4, 4]: exact in fp32
    c = {m.name: m for m in mats}["bf16-384x70-padded"]
    A, B, Ad, Bd = T.mat_operands(c, "exact")
    lay = T.layout(c)
    assert A.shape == (c.R, lay.lda) and bool(torch.isnan(A[:, c.P:].float()).all()) and bool(torch.isnan(B[:, c.Q:].float()).all())
    assert Ad.abs().max() == 4 and bool((Ad == Ad.round()).all()) and Ad.unique().numel() == 9
    g = {x.name: x for x in groups}["fp8-330x100-R384"]
    A, B, ref, sa, sb = T.fp8_single_operands(g, "exact")
    assert A.shape == (384, 336 + 16) and B.shape == (384, 112 + 16)
    a, b = A[:, :330].double(), B[:, :100].double()
    assert a.abs().max() == 4 and b.abs().max() == 8 and bool((a == a.round()).all()) and bool((b == b.round()).all())
    assert 128 * 4 * 8 < 2 ** 13 and bool((ref == ref.round()).all())
    _, _, probs = T.group_operands({x.name: x for x in groups}["fp8-52x1"], "exact")
    assert len(probs) == 52 and all(p[0].stride(0) > 16 * 52 for p in probs) and all(p[0].storage_offset() % 16 == 0 for p in probs)
