"""tests/attention_cases.py on the CPU: for every call of its GRID the attention launch plan (attn_plan of csrc/attention.hip)
equals what the commit before it launched and answered (tests/golden/attn_plan.json, which itself holds every instance, every
return code and every block order at every CU count); the four queries agree with the plan; the instance names the plan returns
are the rows of the instance lists of the two MFMA units, read from the source text, and every unit has one launch site per
pass; the port of attn_item is a bijection for every block order; CASES(ncu) reaches every (order, reason, rotation) and every
(order, instance) pair for several CU counts, each CU-dependent shape inside its own constraint.  The shared reference:
chunked over the batch it is the unchunked one, the bounds it sets fail a zeroed group, and the operands of the cases with few
(batch, head) pairs are well-conditioned for those bounds by a criterion read from the reference alone."""
import ctypes as C
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as A  # noqa: E402
from oracle import rng_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drakegpt_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_plan.json")
NCUS = A.NCUS
UNITS = ("attention.hip", "attention_simple.hip", "attention_mfma.hip", "attention_mfma_doc.hip")
GENERIC = {f"attn_{k}_simple_kernel<{t},{d}>" for k in ("fwd", "bwd_dq", "bwd_dkv") for t in ("float", "bf16_t") for d in ("false", "true")}


def source(name):
    return open(os.path.join(CSRC, name)).read()


def listed_instances():
    """(non-DOC names, DOC names): what the row macros of the two MFMA units make of the instance lists of attention_mfma.hip"""
    text, doc = source("attention_mfma.hip"), source("attention_mfma_doc.hip")
    lists = dict(re.findall(r"#define (ATTN_\w+_INSTANCES)\(X\) (?:\\\n)?((?:.*\\\n)*.*)\n", text))
    assert sorted(lists) == ["ATTN_DKV_INSTANCES", "ATTN_DQ_TILE_INSTANCES", "ATTN_FWD_INSTANCES"]
    assert "#define ATTN_DQ_BOTH(X, KB, F8) X(true, KB, F8, false) X(true, KB, F8, true)\n" in text
    fwd = re.findall(r"X\((\w+), (\w+), (\w+)\)", lists["ATTN_FWD_INSTANCES"])
    dq = [("true", kb, f8, sh) for kb, f8 in re.findall(r"ATTN_DQ_BOTH\(X, (\w+), (\w+)\)", lists["ATTN_DQ_TILE_INSTANCES"]) for sh in ("false", "true")]
    dkv = re.findall(r"X\(([\w<>]+), ATTN_DKV_KEY", lists["ATTN_DKV_INSTANCES"])
    assert len(fwd) == lists["ATTN_FWD_INSTANCES"].count("X(") == 5 and len(dq) == 2 * lists["ATTN_DQ_TILE_INSTANCES"].count("ATTN_DQ_BOTH") == 8
    assert len(dkv) == lists["ATTN_DKV_INSTANCES"].count("X(") == 6
    # the row macros: name and kernel from the same arguments; the recompute dQ instance is the one row written out
    assert '"attn_fwd_mfma_kernel<" #DROP "," #KEEP "," #F8 ">", attn_fwd_mfma_kernel<DROP, KEEP, F8>,' in text
    assert '"attn_bwd_dq_mfma_kernel<" #TILES "," #KB "," #F8 "," #SH ">", attn_bwd_dq_mfma_kernel<TILES, KB, F8, SH>,' in text
    assert "#define ATTN_DKV_ROW(K, KEY, LDS) {KEY, #K, K, LDS}," in text
    assert '"attn_fwd_mfma_kernel<" #DROP "," #KEEP "," #F8 ",true>", attn_fwd_mfma_kernel<DROP, KEEP, F8, true>,' in doc
    assert '"attn_bwd_dq_mfma_kernel<" #TILES "," #KB "," #F8 "," #SH ",true>", attn_bwd_dq_mfma_kernel<TILES, KB, F8, SH, true>,' in doc
    assert re.findall(r"rows\[\] = \{(.*)\};", text) == ["ATTN_FWD_INSTANCES(ATTN_FWD_ROW)", "ATTN_DQ_ROW(false, false, false, false) ATTN_DQ_TILE_INSTANCES(ATTN_DQ_ROW)",
                                                          "ATTN_DKV_INSTANCES(ATTN_DKV_ROW)"]
    assert re.findall(r"rows\[\] = \{(.*)\};", doc) == ["ATTN_FWD_INSTANCES(ATTN_DOC_FWD_ROW)", "ATTN_DQ_TILE_INSTANCES(ATTN_DOC_DQ_ROW)"]
    dq_all = [("false",) * 4] + dq
    plain = {f"attn_fwd_mfma_kernel<{','.join(a)}>" for a in fwd} | {f"attn_bwd_dq_mfma_kernel<{','.join(a)}>" for a in dq_all} | set(dkv)
    docs = {f"attn_fwd_mfma_kernel<{','.join(a)},true>" for a in fwd} | {f"attn_bwd_dq_mfma_kernel<{','.join(a)},true>" for a in dq}
    return plain, docs


def golden():
    g = json.load(open(GOLDEN))
    assert g["grid_sha"] == A.GRID_SHA and g["launch_fields"] == list(A.Launch._fields) and len(g["rows"]) == len(A.GRID)
    launches = [A.Launch(g["names"][l[0]], *l[1:]) for l in g["launches"]]
    return [(r[0], tuple(launches[i] for i in r[1:3] if i >= 0), tuple(r[3:])) for r in g["rows"]]


def all_instances(ncu=256, orders=(0, 1, 2)):
    """{(order, kind, name)} over everything the plan returns for the GPU tests' calls: one shape per order, both dropout settings,
    every form and fp8 setting"""
    shapes = {0: (2, 160, 2), 1: (2, 128, 3), 2: (1, 512, 3)}
    out = set()
    for o in orders:
        B, T, NH = shapes[o]
        assert A.order(B, T, NH, ncu)[0] == o
        for p, form, fp8 in itertools.product((0.0, 0.2), A.FORMS, A.FP8):
            if fp8 and form == "recompute":
                with pytest.raises(ValueError):
                    A.instances(B, T, NH, p, ncu, form, fp8)
                continue
            out |= {(o, kind, n) for kind, n in zip(("fwd", "dq", "dkv"), A.instances(B, T, NH, p, ncu, form, fp8))}
    return out


def reached(cases, ncu):
    """{(order, kind, name)} the GPU tests launch for a case list"""
    out = set()
    for c in cases:
        o = A.order(c.B, c.T, c.NH, ncu)[0]
        for p in c.ps:
            for form, fp8 in A.runs(p, c.fp8):
                out |= {(o, kind, n) for kind, n in zip(("fwd", "dq", "dkv"), A.instances(c.B, c.T, c.NH, p, ncu, form, fp8))}
            # the forward alone, without keep bits (the first launch of every case)
            out.add((o, "fwd", A.instances(c.B, c.T, c.NH, p, ncu, "tiles")[0]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------------------
def test_plan_equals_golden():
    gold = golden()
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "nt_plan.json"))
    bad = []
    for c, (rc, launches, q) in zip(A.GRID, gold):
        p = A.plan(c)
        got = (p.rc, p.launches, (p.mfma_ok, p.fp8_out_ok, p.keep_bytes, p.workspace_bytes))
        if got != (rc, launches, q):
            bad.append((c.name, got, (rc, launches, q)))
        if p.rc:                                             # a refusal launches nothing
            assert p.n_launch == 0 and not p.launches, c.name
        else:
            assert p.family == int(c.dtype == A.BF16 and p.mfma_ok) and p.passes == ((1, 2) if c.bwd else (0,)) and p.block == 256, c.name
    assert not bad, (len(bad), bad[:3])


def test_golden_holds_every_instance_code_and_order():
    """over the golden file itself: a grid too thin to reach an instance, a return code or a block order fails here"""
    gold = golden()
    plain, docs = listed_instances()
    names = {l.name for _, ls, _ in gold for l in ls}
    assert len(plain) == 20 and len(docs) == 13 and names == plain | docs | GENERIC, (plain | docs | GENERIC) ^ names
    assert {rc for rc, _, _ in gold} == {0, -1, -2, -3}
    for ncu in NCUS:
        pairs = {(l.balance, ("length" if l.nblk >= 16 else "size") if l.balance == 2 else None)
                 for c, (_, ls, _) in zip(A.GRID, gold) if c.ncu == ncu for l in ls if l.nblk}
        assert pairs == {(0, None), (1, None), (2, "length"), (2, "size")}, (ncu, pairs)
    # every parameter both ways; the dQ substitution; the tiles behind the delta floats
    for f in "drop keep rng_is_qkv sinv starts".split():
        assert {getattr(l, f) for _, ls, _ in gold for l in ls} == {0, 1}, f
    assert all((l.thr, l.inv_keep, l.site) == (0, A.ONE, 0) for _, ls, _ in gold for l in ls if l.rng_is_qkv)
    assert all(l.tile_off == -1 or (l.tile_off > 0 and l.tile_off % 256 == 0) for _, ls, _ in gold for l in ls)
    assert not any(ls[1].sinv for _, ls, _ in gold if len(ls) == 2) and any(ls[0].sinv for _, ls, _ in gold if len(ls) == 2)
    for f in range(2):
        assert {q[f] for _, _, q in gold} == {0, 1}


def test_queries_agree_with_the_plan():
    """the public entries read the device's CU count (256 without one); their answers do not depend on it"""
    lib = A._lib().lib
    shapes = {(c.B, c.T, c.NH, c.H, c.dtype) for c in A.GRID}
    assert len(shapes) > 50
    for s in shapes:
        for bwd in (0, 1):
            p = A.plan(A.call(bwd, *s, ncu=0))
            assert (lib.dg_attn_fp8_out_supported(*s), lib.dg_attn_keep_bits_bytes(*s), lib.dg_attn_bwd_workspace_bytes(*s)) == \
                   (p.fp8_out_ok, p.keep_bytes, p.workspace_bytes), s
            assert p.fp8_out_ok == int(p.mfma_ok and s[4] == A.BF16) and (p.keep_bytes > 0) == bool(p.fp8_out_ok), s
            B, T, NH = s[:3]
            if min(B, T, NH) > 0:
                assert p.workspace_bytes - (32 * p.keep_bytes) == -(-B * NH * T * 4 // 256) * 256, s
            else:
                assert p.workspace_bytes == 0 and p.keep_bytes == 0


def test_instance_names_are_the_launch_targets_of_the_kernel_file():
    plain, docs = listed_instances()
    targets = plain
    assert len(targets) == 5 + 9 + 6
    assert len([t for t in targets if t.startswith("attn_fwd")]) == 5 and len([t for t in targets if t.startswith("attn_bwd_dq")]) == 9
    assert {n for _, _, n in all_instances()} == targets
    assert len(docs) == 5 + 8 and {n for o in (0, 1, 2) for p in (0.0, 0.2) for form in ("tiles", "keep_bits") for fp8 in A.FP8
                                   for n in A.instances(*{0: (2, 160, 2), 1: (2, 128, 3), 2: (1, 512, 3)}[o], p, 256, form, fp8, doc=True)[:2]} == docs
    # one launch site per pass per unit, each on the row it looked up; the decode kernels keep theirs
    sites = {u: source(u).count("hipLaunchKernelGGL") for u in UNITS}
    assert sites == {"attention.hip": 0, "attention_simple.hip": 3 + 4, "attention_mfma.hip": 3, "attention_mfma_doc.hip": 2}, sites
    for u, n in (("attention_mfma.hip", 3), ("attention_mfma_doc.hip", 2)):
        assert source(u).count("if (r && p) hipLaunchKernelGGL(r->kernel, dim3(grid), dim3(256), r->lds, s, *p);") == n
    simple = source("attention_simple.hip")
    simple = simple[simple.index("int dg_attn_simple_launch("):]
    assert re.findall(r"hipLaunchKernelGGL\(\((\w+)<T, DOC>\)", simple) == ["attn_fwd_simple_kernel", "attn_bwd_dq_simple_kernel", "attn_bwd_dkv_simple_kernel"]
    # the plan is made once per call, and the CU count is read by the extern "C" side only
    text = source("attention.hip")
    assert text.count(" attn_plan(") == 4 and text.count("dg_num_cus()") == 3 and "dg_num_cus" not in text[:text.index("static int attn_run(")]
    assert "attn_mfma_kernel<" not in text and "hipGetDevice" not in "".join(source(u) for u in UNITS)


@pytest.mark.parametrize("args,want", [
    ((2, 256, 3, 256), (1, None)), ((3, 100, 2, 256), (1, None)), ((2, 130, 2, 256), (0, None)), ((1, 1024, 2, 256), (2, "length")),
    ((1, 512, 1, 256), (2, "length")), ((1, 480, 64, 256), (0, None)), ((8, 1024, 16, 256), (2, "length")),
    ((422, 256, 1, 256), (1, None)), ((423, 256, 1, 256), (2, "size")), ((844, 128, 1, 256), (1, None)), ((845, 128, 1, 256), (2, "size")),
    ((64, 256, 6, 256), (1, None)), ((64, 256, 6, 104), (2, "size")), ((8, 384, 16, 64), (2, "size")), ((1, 2, 1, 256), (0, None)),
])
def test_the_restated_order(args, want):
    assert A.order(*args) == want


def test_the_restated_instances():
    I = A.instances
    assert I(2, 256, 3, 0.2, 256, "tiles") == ("attn_fwd_mfma_kernel<true,false,false>", "attn_bwd_dq_mfma_kernel<true,false,false,false>", "attn_bwd_dkv_tiles_shared_kernel")
    assert I(2, 256, 3, 0.2, 256, "keep_bits") == ("attn_fwd_mfma_kernel<true,true,false>", "attn_bwd_dq_mfma_kernel<true,true,false,false>", "attn_bwd_dkv_tiles_shared_kernel")
    assert I(2, 256, 3, 0.0, 256, "keep_bits") == ("attn_fwd_mfma_kernel<false,false,false>", "attn_bwd_dq_mfma_kernel<true,false,false,false>", "attn_bwd_dkv_tiles_shared_kernel")
    assert I(2, 130, 2, 0.2, 256, "recompute") == ("attn_fwd_mfma_kernel<true,false,false>", "attn_bwd_dq_mfma_kernel<false,false,false,false>", "attn_bwd_dkv_mfma_kernel<true>")
    assert I(2, 130, 2, 0.0, 256, "tiles", "both") == ("attn_fwd_mfma_kernel<false,false,true>", "attn_bwd_dq_mfma_kernel<true,false,true,false>", "attn_bwd_dkv_tiles_f8_kernel")
    assert I(1, 1024, 2, 0.1, 256, "keep_bits", "only8") == ("attn_fwd_mfma_kernel<true,true,true>", "attn_bwd_dq_mfma_kernel<true,true,true,true>", "attn_bwd_dkv_tiles_shared_f8_kernel")
    assert I(1, 1024, 2, 0.1, 256, "tiles", "both")[:2] == ("attn_fwd_mfma_kernel<true,true,true>", "attn_bwd_dq_mfma_kernel<true,false,true,true>")
    assert I(1, 1024, 2, 0.1, 256, "recompute")[1:] == ("attn_bwd_dq_mfma_kernel<false,false,false,false>", "attn_bwd_dkv_mfma_kernel<true>")


def test_supported_is_the_librarys_rule():
    assert A.supported(1, 2, 1) and not A.supported(1, 255, 1) and not A.supported(1, 256, 1, 128) and not A.supported(0, 2, 1)
    assert A.supported(1, 65534, 1) and not A.supported(1, 65536, 1) and not A.supported(2, 46342, 1)


# ---------------------------------------------------------------------------------------------------------------------
# attn_item
# ---------------------------------------------------------------------------------------------------------------------
# (B, NH, nblk): grids of 1, 2, 3, 5 (not / 8), 7, 8, 9, 26, 27 workgroups; nblk % 4 != 0 for order 0 only
ITEM_SHAPES = [(1, 1, 1), (2, 3, 1), (3, 3, 3), (2, 2, 5), (1, 1, 4), (1, 3, 4), (5, 1, 4), (7, 1, 8), (3, 3, 4), (13, 1, 8), (3, 9, 4),
               (1, 1, 16), (1, 3, 16), (5, 7, 12), (107, 3, 8), (37, 23, 4), (141, 3, 8), (9, 7, 20)]


@pytest.mark.parametrize("ncu", NCUS + (1, 3))
@pytest.mark.parametrize("order", [0, 1, 2])
def test_item_maps_the_valid_waves_onto_every_block_once(order, ncu):
    """every order (whatever fill would have chosen: the kernels' arithmetic must hold for each), every shape: the valid
    (blockIdx, wave) pairs cover every (bh, blk) exactly once; in orders 1 and 2 a workgroup's four waves share one bh and are
    valid together (the shared-tile kernels rely on both)"""
    for B, NH, nblk in ITEM_SHAPES:
        if order and nblk % 4:
            continue
        grid = (B * NH * nblk + 3) // 4
        seen = np.zeros((B * NH, nblk), dtype=np.int64)
        n_invalid = 0
        for wg in range(grid):
            got = [A.item(order, wg, w, B, NH, nblk, ncu, grid) for w in range(4)]
            if order:
                assert len({bh for bh, _, _ in got}) == 1 and len({v for _, _, v in got}) == 1, (B, NH, nblk, wg, got)
                assert len({blk for _, blk, _ in got}) == 4
            for bh, blk, valid in got:
                if valid:
                    assert 0 <= bh < B * NH and 0 <= blk < nblk, (B, NH, nblk, wg, got)
                    seen[bh, blk] += 1
                else:
                    n_invalid += 1
        assert (seen == 1).all(), (order, ncu, B, NH, nblk)
        assert n_invalid == 4 * grid - B * NH * nblk and (order == 0 or n_invalid == 0)


def test_item_rotation_slots_and_pairs():
    """order 1 at nblk = 8 (wpq = 2): workgroup g of a pair takes the blocks {7 - g, g, 5 - g, g + 2} -- two pairs of cost 9 --
    and the rotation only permutes them among the waves"""
    B, NH, nblk, ncu = 40, 1, 8, 16
    grid = B * NH * nblk // 4
    slots = {0: (0, 1, 2, 3), 1: (1, 0, 2, 3), 2: (1, 2, 3, 0)}
    assert {(wg // ncu) % 3 for wg in range(grid)} == {0, 1, 2}
    for wg in range(grid):
        g = A.xcd_remap(wg, grid) % 2
        base = (7 - g, g, 5 - g, g + 2)
        blks = tuple(A.item(1, wg, w, B, NH, nblk, ncu, grid)[1] for w in range(4))
        assert blks == tuple(base[s] for s in slots[(wg // ncu) % 3]), (wg, blks)
    # order 2: class c takes the four blocks 4 c .. 4 c + 3 from the heavy end, all heads of class 0 first
    assert [A.item(2, 3 + 5 * c, w, 5, 1, 8, ncu, 10)[:2] for c in (0, 1) for w in range(4)] == [(3, b) for b in (7, 6, 5, 4, 3, 2, 1, 0)]
    # order 0: four consecutive items, the last workgroup ragged
    assert [A.item(0, 6, w, 3, 3, 3, ncu, 7) for w in range(4)] == [(8, 0, True), (8, 1, True), (8, 2, True), (9, 0, False)]


def test_xcd_remap_is_a_permutation_that_groups_by_xcd():
    for n in list(range(1, 70)) + [162, 270, 516, 642, 762, 851]:
        m = [A.xcd_remap(i, n) for i in range(n)]
        assert sorted(m) == list(range(n))
        for x in range(min(8, n)):                         # the workgroups of XCD x (blockIdx % 8 == x) get consecutive ids
            ids = m[x::8]
            assert ids == list(range(ids[0], ids[0] + len(ids)))


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncu", NCUS)
def test_cases_reach_what_they_are_named_for(ncu):
    cases = A.CASES(ncu)
    assert [c.name for c in cases] == A.NAMES and len(set(A.NAMES)) == len(A.NAMES)
    for c in cases:
        assert A.supported(c.B, c.T, c.NH) and c.T % 2 == 0, c
        assert A.order(c.B, c.T, c.NH, ncu) == (c.order, c.reason), c
        assert A.rotations(c.B, c.T, c.NH, ncu) == c.rotations, c
        assert c.B * c.NH * c.T * c.T < 2 ** 31                      # (rng_ref.keep_mask's index range, with room)
    by = {c.name: c for c in cases}
    lim = A.size_limit(ncu)
    # the CU-dependent shapes satisfy their own constraints
    r = by["rotation"]
    g = A.grid(r.B, r.T, r.NH)
    assert g == 2 * r.B * r.NH and 2 * ncu < g <= lim and g % 8 != 0 and A.blocks(r.T) == 8 and r.T % 32 != 0
    assert g - 2 * ncu >= ncu // 4                                   # the third round is no token
    s4 = by["heavy-size-4"]
    assert s4.B * s4.NH > lim and s4.B * s4.NH % 8 != 0 and A.blocks(s4.T) == 4 and s4.T % 32 != 0
    s8 = by["heavy-size-8"]
    assert 2 * s8.B * s8.NH > lim >= 2 * (s8.B * s8.NH - 1) and A.blocks(s8.T) == 8
    # the fixed shapes
    assert [by[n].invalid_waves for n in ("one-tile-2", "one-tile-32", "plain-ragged", "plain-5-blocks")] == [3, 2, 1, 0]
    assert by["plain-ragged"].n_items == 27 and A.blocks(66) == 3 and 66 % 32 == 2 and A.blocks(482) == 16 and 482 % 32 == 2
    assert all(A.blocks(by[n].T) == 16 for n in ("heavy-length", "heavy-length-ragged"))


def test_case_shapes_at_256_cus():
    by = {c.name: c for c in A.CASES(256)}
    assert (by["rotation"].B, A.grid(by["rotation"].B, 250, 3)) == (107, 642)
    assert (by["heavy-size-4"].B, by["heavy-size-4"].T, by["heavy-size-4"].NH) == (37, 126, 23) and A.grid(37, 126, 23) == 851
    assert by["heavy-size-8"].B * by["heavy-size-8"].NH == 423


@pytest.mark.parametrize("ncu", NCUS)
def test_cases_cover_every_order_reason_rotation_and_instance(ncu):
    cases = A.CASES(ncu)
    assert {(c.order, c.reason) for c in cases} == {(0, None), (1, None), (2, "length"), (2, "size")}
    assert set().union(*(c.rotations for c in cases)) == {0, 1, 2}
    got = reached(cases, ncu)
    assert got == all_instances(ncu), sorted(all_instances(ncu) - got)
    assert {n for _, _, n in got} == listed_instances()[0]
    # what the suite did not reach before, by name
    by = {c.name: c for c in cases}
    ins = lambda name, p, form, fp8=None: A.instances(by[name].B, by[name].T, by[name].NH, p, ncu, form, fp8)

    def launched(name, p, form, fp8=None):
        c = by[name]
        return p in c.ps and (form, fp8) in A.runs(p, c.fp8)

    # order 0 with dropout on the MFMA path, with invalid waves in the last workgroup
    for name in ("one-tile-32", "plain-ragged"):
        assert by[name].invalid_waves > 0 and by[name].order == 0 and all(launched(name, 0.2, f) for f in A.FORMS)
    assert ins("plain-ragged", 0.2, "keep_bits")[:2] == ("attn_fwd_mfma_kernel<true,true,false>", "attn_bwd_dq_mfma_kernel<true,true,false,false>")
    assert ins("plain-ragged", 0.2, "recompute")[1:] == ("attn_bwd_dq_mfma_kernel<false,false,false,false>", "attn_bwd_dkv_mfma_kernel<true>")
    # order 0 through the fp8 entry points
    assert launched("plain-5-blocks", 0.0, "tiles", "both") and launched("plain-5-blocks", 0.2, "keep_bits", "only8")
    assert ins("plain-5-blocks", 0.2, "keep_bits", "both") == ("attn_fwd_mfma_kernel<true,true,true>", "attn_bwd_dq_mfma_kernel<true,true,true,false>", "attn_bwd_dkv_tiles_f8_kernel")
    assert ins("plain-5-blocks", 0.0, "tiles", "both")[:2] == ("attn_fwd_mfma_kernel<false,false,true>", "attn_bwd_dq_mfma_kernel<true,false,true,false>")
    # order 2 by length: the hashed and the recompute forms with dropout, a ragged last tile
    for name in ("heavy-length", "heavy-length-ragged"):
        assert all(launched(name, 0.2, f) for f in A.FORMS)
        assert ins(name, 0.2, "tiles")[1] == "attn_bwd_dq_mfma_kernel<true,false,false,true>"
    # order 2 by size at four and at eight blocks, all forms; fp8 on one of them and on the rotation case
    assert all(launched("heavy-size-4", 0.2, f) for f in A.FORMS) and all(launched("heavy-size-8", 0.0, f) for f in A.FORMS)
    assert launched("heavy-size-4", 0.2, "keep_bits", "both") and launched("rotation", 0.2, "keep_bits", "only8")
    assert ins("heavy-size-4", 0.2, "keep_bits", "both")[1:] == ("attn_bwd_dq_mfma_kernel<true,true,true,true>", "attn_bwd_dkv_tiles_shared_f8_kernel")
    assert all(launched("rotation", 0.2, f) for f in A.FORMS) and ins("rotation", 0.2, "tiles")[2] == "attn_bwd_dkv_tiles_shared_kernel"
    # the smallest supported shapes
    assert (by["one-tile-2"].T, by["one-tile-32"].T) == (2, 32)


def test_the_coverage_check_notices_a_missing_case():
    """without its only case an (order, instance) pair is named"""
    for drop in ("plain-5-blocks", "pairs-small", "rotation", "heavy-length"):
        cases = [c for c in A.CASES(256) if c.name != drop]
        assert all_instances(256) - reached(cases, 256), drop


def test_rotation_case_puts_every_rotation_on_every_kind_of_head():
    """at 256 CUs: each rotation k serves whole (batch, head) pairs, both workgroups g = 0 / 1 of some pair, and the heads the
    invariance test singles out (lowest and highest bh) lie in different rotations"""
    c = A.case("rotation", 256)
    g = A.grid(c.B, c.T, c.NH)
    rot_of = {}
    for wg in range(g):
        bh = A.item(1, wg, 0, c.B, c.NH, 8, 256, g)[0]
        rot_of.setdefault(bh, set()).add((wg // 256) % 3)
    assert set().union(*rot_of.values()) == {0, 1, 2}
    assert all(any(k in v for v in rot_of.values()) for k in (0, 1, 2))
    assert rot_of[0] != rot_of[c.B * c.NH - 1]


# ---------------------------------------------------------------------------------------------------------------------
# the shared reference
# ---------------------------------------------------------------------------------------------------------------------
def test_keep_slab_is_keep_mask():
    full = rng_ref.keep_mask(A.SEED, A.STEP, A.SITE, 0.2, 5000)
    assert np.array_equal(A.keep_slab(0.2, 0, 5000), full) and np.array_equal(A.keep_slab(0.2, 1234, 4001), full[1234:4001])


def test_the_bounds_of_the_small_cases_mean_something():
    """every (row, head) bound of dk and dv lies below 0.1 -- a zeroed or misplaced group (error 1) fails it --, dq's too
    from query row 48 on, the last 8 rows at T = 32 (the first rows' dq cancels: oracle/parity.py,
    attention_bwd_bounds_by_position; the invariance and keep-bits comparisons have no such blind rows); the two-row case
    included, whose dq needs the denominator floor (its first group is exactly zero, and so is the median of its two)"""
    for c in A.CASES(256):
        if c.B * c.NH > 6:
            continue
        for p in c.ps:
            R = A.reference(c.B, c.T, c.NH, p, c.draw)
            assert A.dq_conditioning(R, c.B, c.T, c.NH) < 1, (c.name, p, A.dq_conditioning(R, c.B, c.T, c.NH))
            assert (R["floors"]["dq"] > 1) == (c.T == 2) and R["floors"]["dk"] == R["floors"]["dv"] == 0, (c.name, R["floors"])
            for n in ("dq", "dk", "dv"):
                b = R["bounds"][n].view(c.B, c.T, c.NH)
                assert b.max().item() < (2 if n == "dq" else 0.1), (c.name, p, n, b.max().item())
                first = 0 if c.T == 2 else min(48, c.T - 8)          # (a bound is the worst of the 16 rows either side: T = 32 keeps 8 rows clear of row 0's)
                assert b[:, first:].max().item() < 0.1, (c.name, p, n, b[:, first:].max().item())
    A.reference.cache_clear()


def test_the_conditioning_criterion_names_the_draw_that_was_replaced():
    """attention_cases.DRAW: draw 0 of the ragged 16-block case without dropout has a group of dq -- head 2, query row 1 -- whose
    inherited error is six times what its bound allows for; the draw in use has none.  Read from the reference alone."""
    c = A.case("heavy-length-ragged", 256)
    assert c.draw == 1 and all(x.draw == 0 for x in A.CASES(256) if x.name != c.name)
    R = A.reference(c.B, c.T, c.NH, 0.0, 0)
    assert 5 < A.dq_conditioning(R, c.B, c.T, c.NH) < 7
    den = R["dq"].reshape(-1, 64).norm(dim=1)
    den = den.clamp_min(0.1 * den.median().item()).view(c.T, c.NH)          # (rowwise_rel's denominators)
    sig = R["delta_noise"][0].t() / den
    assert int(sig.argmax()) == 1 * c.NH + 2 and 0.08 < sig[1, 2].item() < 0.11 and R["bounds"]["dq"].view(c.T, c.NH)[1, 2].item() < 0.05
    A.reference.cache_clear()


def test_chunked_reference_is_the_unchunked_one(monkeypatch):
    import torch
    from oracle import parity as P
    B, T, NH, p = 3, 66, 3, 0.2
    whole = dict(A.reference(B, T, NH, p))
    A.reference.cache_clear()
    monkeypatch.setattr(A, "CHUNK_ELEMS", NH * T * T)                 # one batch entry per chunk
    parts = A.reference(B, T, NH, p)
    A.reference.cache_clear()
    keep = torch.from_numpy(rng_ref.keep_mask(A.SEED, A.STEP, A.SITE, p, B * NH * T * T).reshape(B, NH, T, T)).double()
    R = P.attention_fp64(whole["qkv"], whole["dout"], B, T, NH, 64, keep, p)
    M = P.attention_fp64(whole["qkv"], whole["dout"], B, T, NH, 64, keep, p, model=True)
    bounds = P.attention_bwd_bounds_by_position(R, M, B, T, NH, 64)
    for ref in (whole, parts):
        for k in ("out", "lse", "dq", "dk", "dv"):
            assert torch.equal(ref[k], R[k]), k
        assert torch.equal(ref["env"], P.attention_fwd_envelope(R))
        for k in ("dq", "dk", "dv"):
            assert torch.equal(ref["bounds"][k], bounds[k]), k
        assert int(ref["dead"].sum()) > 0 and ref["dead"].shape == (B, NH, T)
