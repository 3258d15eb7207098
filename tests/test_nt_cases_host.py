"""The NT GEMM launch plan (nt_plan of csrc/gemm.hip) on the CPU: for every case of tests/nt_cases.py the plan equals what the
commit before it launched and answered (tests/golden/nt_plan.json); the five public query entries agree with the plan; the
instance names the plan returns are the rows of the one instance list in csrc/gemm_nt_ws.h, read from the source text; every
translation unit has one launch site; a handful of plans written out by hand."""
import ctypes as C
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nt_cases as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drakegpt_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "nt_plan.json")
STAGED = {"gemm_nt_kernel<float,float>", "gemm_nt_kernel<bf16_t,float>", "gemm_nt_kernel<bf16_t,bf16_t>", "gemm_nt_x3_kernel"}


def source(name):
    return open(os.path.join(CSRC, name)).read()


def listed_instances():
    """the names NT_WS_ROW gives the rows of the instance lists of gemm_nt_ws.h, by list"""
    text = source("gemm_nt_ws.h")
    assert '"gemm_nt_ws_kernel<" #TO "," #PF "," #NJ "," #EPI "," #F8 ">", gemm_nt_ws_kernel<TO, PF, NJ, EPI, F8>}' in text
    assert "#define NT_WS_BOTH(X, TO, PF, EPI, F8) X(TO, PF, 4, EPI, F8) X(TO, PF, 6, EPI, F8)\n" in text
    out = {}
    for lst, body in re.findall(r"#define NT_WS_INSTANCES_(\w+)\(X\) \\\n((?:.*\\\n)*.*)\n", text):
        rows = re.findall(r"NT_WS_BOTH\(X, (\w+), (\w+), (\d), (\d)\)", body)
        assert len(rows) == body.count("NT_WS_BOTH") and len(set(rows)) == len(rows), lst
        out[lst] = {f"gemm_nt_ws_kernel<{to},{pf},{nj},{epi},{f8}>" for to, pf, epi, f8 in rows for nj in (4, 6)}
    return out


def golden_rows():
    g = json.load(open(GOLDEN))
    assert g["grid_sha"] == T.GRID_SHA and g["fields"] == list(T.Row._fields) and len(g["rows"]) == len(T.GRID)
    return [T.Row(r[0], g["names"][r[1]], *r[2:]) for r in g["rows"]]


def test_plan_equals_golden():
    gold = golden_rows()
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "generate_launches.json"))
    bad = []
    for case, want in zip(T.GRID, gold):
        p = T.plan(case)
        if T.row_of(p) != want:
            bad.append((case.name, T.row_of(p), want))
            continue
        # the instance fields are the name's
        if p.rc == 0:
            parsed = T.parse_name(p.name)
            assert (p.family,) == parsed[:1] and (p.family != 0 or (p.family, p.out_dtype, p.pf, p.nj, p.epi, p.f8) == parsed), case.name
            assert p.family != 0 or (p.bn == 32 * p.nj and p.block == 768 and p.grid == min(p.n_tiles, case.ncu)), case.name
        else:
            assert p.name == "" and not any(getattr(p, f) for f in T.LAUNCH_FIELDS.split()), case.name
    assert not bad, (len(bad), bad[:5])
    # what the grid holds: every pairing, every named form on every family that has it, every refusal, both cs_accum values,
    # every flag both ways
    ok = [(c, r) for c, r in zip(T.GRID, gold) if r.rc == 0]
    assert {(c.ind, c.outd) for c, _ in ok} == set(T.PAIRS)
    assert {r.rc for r in gold} == {0, -1, -2, -3}
    for f in "cs_accum vec_ok mask_vec_ok warm_b drop q8_only sign_ok colsum_ok fp8_out_ok".split():
        assert {bool(getattr(r, f)) for _, r in ok} == {False, True}, f
    assert {c.ncu for c, r in ok if r.fp8_out_ok} == {256} and {c.ncu for c, r in ok if r.cs_accum} == set(T.NCUS)
    late = [c for c, r in zip(T.GRID, gold) if r.rc == -1 and c.ind == T.E4M3 and c.opts == ("sign_bits",) and not c.over]
    assert late                                              # valid by every check, refused for want of an instance


def test_queries_agree_with_the_plan():
    """the public entries read the device's CU count (256 without one) and the library's own stamp-buffer state (none)"""
    L = T._lib()
    lib = L.lib
    n = 0
    for case in T.GRID:
        a = case.args()
        p = T.plan_of(a, 0, 0)
        if p.rc != 0:
            continue
        n += 1
        ref = C.byref(a)
        assert (lib.dg_gemm_nt_sign_bits_supported(ref), lib.dg_gemm_nt_colsum_supported(ref), lib.dg_gemm_nt_colsum_rows(ref),
                lib.dg_gemm_nt_fp8_out_supported(ref), lib.dg_gemm_nt_sign_bits_bytes(a.M, a.N)) == \
               (p.sign_ok, p.colsum_ok, p.colsum_rows, p.fp8_out_ok, p.sign_bits_bytes), case.name
        # as drakegpt_amd/ops.py asks: a struct that holds the shape, the dtypes and the options' presence only
        q = L.GemmNtArgs()
        q.M, q.N, q.K, q.in_dtype, q.out_dtype = 128, a.N, a.K, a.in_dtype, a.out_dtype
        assert lib.dg_gemm_nt_sign_bits_supported(C.byref(q)) == p.sign_ok, case.name
        if "colsum" in case.opts:                            # ops.gemm_nt_colsum_rows
            q = L.GemmNtArgs()
            q.M, q.N, q.K, q.in_dtype, q.out_dtype, q.ldc, q.sign_bits = a.M, a.N, a.K, a.in_dtype, a.out_dtype, a.N, 16
            assert lib.dg_gemm_nt_colsum_rows(C.byref(q)) == p.colsum_rows > 0, case.name
        if "fp8_out" in case.opts:                           # ops.gemm_nt_fp8_out_supported
            q = L.GemmNtArgs()
            q.M, q.N, q.K, q.in_dtype, q.out_dtype, q.ldc, q.C = a.M, a.N, a.K, a.in_dtype, T.BF16, a.N, 16
            if a.in_dtype == T.E5M2:
                q.sign_bits = q.colsum_part = 16
            else:
                q.bias = q.sign_bits_out = 16
                q.relu = 1
            assert lib.dg_gemm_nt_fp8_out_supported(C.byref(q)) == p.fp8_out_ok == 1, case.name
        if {"sign_bits", "sign_bits_out"} & set(case.opts):
            assert p.sign_ok and a.sign_bits_bytes >= p.sign_bits_bytes
    assert n > 1500
    assert lib.dg_gemm_nt_sign_bits_supported(None) == 0 and lib.dg_gemm_nt_colsum_rows(None) == 0
    assert lib.dg_gemm_nt_colsum_supported(None) == 0 and lib.dg_gemm_nt_fp8_out_supported(None) == 0


def test_plan_names_are_the_listed_instances():
    listed = listed_instances()
    assert sorted(listed) == ["BF16", "E4M3", "E5M2", "X3"] and [len(listed[k]) for k in sorted(listed)] == [30, 20, 14, 10]
    every = set().union(*listed.values())
    assert len(every) == 74
    got = {T.plan(c).name for c in T.GRID} - {""}
    assert got - STAGED <= every, got - STAGED - every
    assert got == every | STAGED, (every | STAGED) - got      # no instance is unreachable
    # a unit expands the lists of its own F8 and no other
    for unit, lists in (("gemm.hip", ["BF16"]), ("gemm_fp8.hip", ["E4M3", "E5M2"]), ("gemm_x3.hip", ["X3"])):
        assert re.findall(r"NT_WS_INSTANCES_(\w+)\(NT_WS_ROW\)", source(unit)) == lists, unit
    for k, f8 in (("BF16", "0"), ("E4M3", "1"), ("E5M2", "2"), ("X3", "3")):
        assert {n[-2] for n in listed[k]} == {f8}
    # the register-staged kernels: name and address out of one expansion as well
    text = source("gemm.hip")
    assert "#define NT_STAGED_ROW(...) {#__VA_ARGS__, __VA_ARGS__}" in text
    assert set(re.findall(r"NT_STAGED_ROW\((gemm_nt_[^()]+)\)", text)) == STAGED


def test_one_launch_site_per_unit():
    for unit in ("gemm_fp8.hip", "gemm_x3.hip"):
        text = source(unit)
        assert text.count("hipLaunchKernelGGL") == 1 and "hipLaunchKernelGGL(r.kernel," in text, unit
        assert "epi ==" not in text
    text = source("gemm.hip")
    nt = text[text.index("// NT launch plan."):text.index('extern "C" int dg_debug_nt_plan(')]
    assert nt.count("hipLaunchKernelGGL") == 2 and nt.count("hipLaunchKernelGGL(r.kernel,") == 1       # + the register-staged kernels'
    assert "epi ==" not in text and "gemm_nt_ws_kernel<" not in text and "gemm_nt_ws_kernel<" not in source("gemm_fp8.hip") + source("gemm_x3.hip")
    body = text[text.index('extern "C" int dg_gemm_nt('):text.index('extern "C" int dg_debug_nt_plan(')]
    assert body.count("nt_plan(") == 1 and body.count("hipLaunchKernelGGL") == 1 and body.count("nt_ws_instance(pl.inst, &p") == 1
    # the CU count and the stamp buffer are read by the extern "C" entries only
    helpers = nt[:nt.index('extern "C" int dg_gemm_nt_sign_bits_supported(')]
    assert "static NtPlan nt_plan(" in helpers and "dg_num_cus" not in helpers and "g_stamp_buffer" not in helpers
    entries = nt[len(helpers):]
    assert entries.count("nt_plan(*a, dg_num_cus(), g_stamp_buffer != nullptr)") == entries.count("dg_num_cus") == 5
    assert len(re.findall(r"^\S.*\) \{$", entries, re.M)) == len(re.findall(r'^extern "C" .*\) \{$', entries, re.M)) == 5


def _bf16(M, N, K, opts=(), ncu=256, **over):
    return T.plan(T.Case("", T.BF16, T.BF16, M, N, K, tuple(opts), ncu, 0, tuple(over.items())))


def test_plan_values():
    ws = "gemm_nt_ws_kernel<%s>"
    # the headline shapes: wide tiles, an exact number of rounds on 256 CUs; weights warm up to 2 MB
    for N, K, tiles, warm in ((384, 384, 256, 1), (1152, 384, 768, 1), (1536, 384, 1024, 1), (384, 1536, 256, 1), (1152, 1536, 768, 0), (1536, 1536, 1024, 0)):
        p = _bf16(16384, N, K)
        assert (p.rc, p.name, p.grid, p.block, p.K, p.tiles_n, p.n_tiles, p.bn) == (0, ws % "bf16_t,false,6,1,0", 256, 768, K, N // 192, tiles, 192), (N, K)
        assert (p.vec_ok, p.mask_vec_ok, p.warm_b, p.drop, p.q8_only) == (1, 0, warm, 0, 0), (N, K)
        assert p.cs_accum == (1 if 32 % (N // 192) == 0 else 0)
        assert p.sign_bits_bytes == 16384 * N // 8 and p.sign_ok == 1 and p.colsum_ok == 0 and p.fp8_out_ok == 0
    p = _bf16(16384, 1536, 384, T.FORMS[2])
    assert p.name == ws % "bf16_t,false,6,2,0"
    p = _bf16(16384, 1536, 384, T.FORMS[3])
    assert p.name == ws % "bf16_t,false,6,3,0" and p.drop == 1
    p = _bf16(16384, 384, 1536, T.FORMS[6])
    assert (p.name, p.colsum_ok, p.colsum_rows, p.cs_accum) == (ws % "bf16_t,true,6,6,0", 1, 512, 1)     # 4 x 256 workgroups / 2 column blocks
    p = _bf16(8192, 1152, 384, T.FORMS[6])
    assert (p.colsum_rows, p.cs_accum, p.n_tiles) == (256, 0, 384)                                       # 32 % 6: one partial row per 32 rows of C
    p = _bf16(8192, 1152, 384, T.FORMS[6], ncu=304)
    assert (p.grid, p.colsum_rows, p.cs_accum) == (304, 256, 0)
    # tile kinds, the register-staged kernel below K = 128 or off whole 64-element steps
    p = _bf16(200, 200, 256)
    assert (p.name, p.grid, p.tiles_n, p.n_tiles, p.bn, p.sign_bits_bytes) == (ws % "bf16_t,false,4,1,0", 4, 2, 4, 128, 4 * 2048)
    p = _bf16(200, 200, 120)
    assert (p.name, p.family, p.grid, p.block, p.cs_accum) == ("gemm_nt_kernel<bf16_t,bf16_t>", 1, 4, 256, 0)
    # fp8: K in 2-byte units; the e4m3 copy on exactly 256 CUs with at least 256 whole tiles
    c = T.Case("", T.E4M3, T.BF16, 4096, 1536, 256, T.FORMS[8], 256, 0, ())
    p = T.plan(c)
    assert (p.name, p.K, p.grid, p.fp8_out_ok, p.n_tiles) == (ws % "bf16_t,false,6,8,1", 128, 256, 1, 256)
    assert T.plan(c._replace(ncu=304)).rc == -1 and T.plan(c._replace(M=3968)).rc == -1
    # the fallback rule: exact, else EPI 0, else that without the prefetch; e4m3 with a prefetchable mask is refused
    p = T.plan(T.Case("", T.E4M3, T.F32, 256, 192, 256, T.FORMS[5], 256, 0, ()))
    assert p.name == ws % "float,false,6,0,1"
    p = T.plan(T.Case("", T.E5M2, T.F32, 256, 192, 256, T.FORMS[4], 256, 0, ()))
    assert p.name == ws % "float,false,6,0,2"
    p = T.plan(T.Case("", T.E5M2, T.BF16, 256, 192, 256, ("sign_bits", "bias"), 256, 0, ()))
    assert p.name == ws % "bf16_t,true,6,0,2"
    assert T.plan(T.Case("", T.E4M3, T.BF16, 256, 192, 256, T.FORMS[4], 256, 0, ())).rc == -1
    # split bf16: K in 2-byte units on the wave-specialised kernel, its own staged kernel otherwise
    p = T.plan(T.Case("", T.X3, T.F32, 256, 192, 256, T.FORMS[7], 256, 0, ()))
    assert (p.name, p.K) == (ws % "float,false,6,7,3", 512)
    p = T.plan(T.Case("", T.X3, T.F32, 256, 192, 100, (), 256, 0, ()))
    assert (p.name, p.family, p.K, p.tiles_n) == ("gemm_nt_x3_kernel", 2, 100, 2)
    # 0 CUs: the device's count, 256 without one
    assert T.plan_of(T.Case("", T.BF16, T.BF16, 16384, 384, 384, (), 0, 0, ()).args(), 0, 0).grid <= 256
