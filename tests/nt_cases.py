"""The NT GEMM launch plan of csrc/gemm.hip (nt_plan): the case grid of tests/test_nt_cases_host.py -- TEST INFRASTRUCTURE (CPU).

dg_gemm_nt launches what nt_plan returns, and the library reports that plan through the diagnostic entry dg_debug_nt_plan: pure
host code that never launches, so the argument structs below carry made-up addresses (aligned or misaligned on purpose, never
dereferenced) and nothing here needs a GPU.  dg_gemm_nt itself is never called on a case: a valid one would launch.

tests/golden/nt_plan.json holds, for every case of GRID in order, what the commit BEFORE nt_plan existed did for the same
arguments: its return code, the kernel instance it launched with grid and block, the host-decided NtParams fields, and what
its five query entries answered.  It was recorded from that commit's own dg_gemm_nt with the launches of the three NT
translation units replaced by a recorder (the kernel expression as spelled at the launch site, normalised to the spelling of
NtWsInstance names), not from the code under test; "grid_sha" ties it to GRID, which therefore changes only together with a new
recording from that commit."""
import collections
import ctypes as C
import functools
import hashlib
import re

F32, BF16, E4M3, E5M2, X3 = 0, 1, 2, 3, 4
DT_NAME = {F32: "f32", BF16: "bf16", E4M3: "e4m3", E5M2: "e5m2", X3: "x3"}
PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32), (X3, F32), (E4M3, BF16), (E4M3, F32), (E5M2, BF16), (E5M2, F32))
ESZ = {F32: 4, BF16: 2, E4M3: 1, E5M2: 1, X3: 4}
NCUS = (256, 304, 64)

# made-up addresses, 128-byte aligned and distinct
ADDR = dict(A=0x1000000, B=0x2000000, C=0x3000000, bias=0x4000000, relu_mask=0x5000000, residual=0x6000000, rng_state=0x7000000,
            sign_bits=0x8000000, sign_bits_out=0x9000000, colsum_part=0xA000000, scale_a=0xB000000, scale_b=0xB000100,
            fp8_out=0xC000000, fp8_out_parts2=0xD000000, fp8_out_step=0xD001000, fp8_out_scale_inv=0xD002000)
OPTIONS = ("bias", "relu", "relu_mask", "drop", "residual", "sign_bits", "sign_bits_out", "colsum", "fp8_out", "fp8_out_only")

# the nine named epilogue forms (EPI of gemm_nt_ws_kernel) by the options that select them
FORMS = {
    1: (),
    2: ("bias", "relu", "sign_bits_out"),
    3: ("bias", "drop", "residual"),
    4: ("sign_bits",),
    5: ("bias",),
    6: ("sign_bits", "colsum"),
    7: ("bias", "residual"),
    8: ("bias", "relu", "sign_bits_out", "fp8_out"),
    9: ("sign_bits", "colsum", "fp8_out"),
}
# combinations that are none of them: EPI 0 (or a refusal) everywhere
OFF_FORMS = (("relu",), ("bias", "relu"), ("residual",), ("relu_mask",), ("drop",), ("sign_bits", "bias"), ("sign_bits_out",),
             ("bias", "relu", "sign_bits_out", "residual"), ("sign_bits", "residual"), ("bias", "drop", "residual", "relu"))


class Case(collections.namedtuple("Case", "name ind outd M N K opts ncu stamps over")):
    """one dg_gemm_nt call: operand / output dtype codes, shape, the options present, the CU count and stamp-buffer state it is
    planned for, and raw overrides of dg_gemm_nt_args fields (applied last)"""
    __slots__ = ()

    def args(self):
        from drakegpt_amd._lib import GemmNtArgs
        a = GemmNtArgs()
        a.A, a.lda, a.B, a.ldb, a.C, a.ldc = ADDR["A"], self.K, ADDR["B"], self.K, ADDR["C"], self.N
        a.M, a.N, a.K, a.in_dtype, a.out_dtype = self.M, self.N, self.K, self.ind, self.outd
        if self.ind in (E4M3, E5M2):
            a.b_dtype, a.scale_a, a.scale_b = E4M3, ADDR["scale_a"], ADDR["scale_b"]
        o = self.opts
        assert set(o) <= set(OPTIONS), o
        if "bias" in o:
            a.bias = ADDR["bias"]
        a.relu = int("relu" in o)
        if "relu_mask" in o:
            a.relu_mask, a.ldmask = ADDR["relu_mask"], self.N
        if "residual" in o:
            a.residual, a.ldr = ADDR["residual"], self.N
        if "drop" in o:
            a.dropout_p, a.rng_state, a.site = 0.25, ADDR["rng_state"], 3
        for k in ("sign_bits", "sign_bits_out"):
            if k in o:
                setattr(a, k, ADDR[k])
                a.sign_bits_bytes = 1 << 40
        if "colsum" in o:
            a.colsum_part, a.colsum_ld, a.colsum_rows = ADDR["colsum_part"], self.N, 1 << 20
        if "fp8_out" in o:
            a.fp8_out, a.ld_fp8_out = ADDR["fp8_out"], self.N
            a.fp8_out_parts2, a.fp8_out_step, a.fp8_out_scale_inv = ADDR["fp8_out_parts2"], ADDR["fp8_out_step"], ADDR["fp8_out_scale_inv"]
            a.fp8_out_only = int("fp8_out_only" in o)
        for k, v in self.over:
            setattr(a, k, v)
        return a


def _grid():
    out, seen = [], set()

    def add(ind, outd, M, N, K, opts=(), ncu=256, stamps=0, **over):
        name = f"{DT_NAME[ind]}>{DT_NAME[outd]}/{'+'.join(opts) or 'plain'}/{M}x{N}x{K}/cu{ncu}" + ("/stamps" if stamps else "")
        name += "".join(f"/{k}={v:#x}" if isinstance(v, int) and v > 4096 else f"/{k}={v}" for k, v in sorted(over.items()))
        if name not in seen:
            seen.add(name)
            out.append(Case(name, ind, outd, M, N, K, tuple(opts), ncu, stamps, tuple(sorted(over.items()))))

    every_form = list(FORMS.values()) + list(OFF_FORMS)
    # every pairing x every form and off-form x every tile kind: square, wide, ragged edge; M whole, and ragged on the named forms
    for ind, outd in PAIRS:
        for opts in every_form:
            for N in (64, 128, 192, 200, 384, 1152):
                add(ind, outd, 256, N, 256, opts)
        for opts in FORMS.values():
            for N in (192, 200):
                add(ind, outd, 200, N, 256, opts)
    # K on both sides of every threshold: K % 64, K >= 128 (bf16), K % 128, K >= 256 (fp8), K % 32, K >= 128 (split), and K that
    # is no whole 16-byte chunk
    for ind, outd in PAIRS:
        for opts in (FORMS[1], FORMS[2], FORMS[4]):
            for K in (8, 32, 64, 96, 100, 120, 128, 160, 192, 256, 288, 320, 384, 512):
                add(ind, outd, 256, 192, K, opts)
    # CU counts: cs_accum both ways, the fp8 copy offered (256 CUs, >= 256 whole tiles) and not; the headline shapes
    shapes = [(4096, 1536, 256), (4096, 1024, 256), (256, 384, 256), (8192, 1152, 384), (4000, 1536, 256)]
    shapes += [(16384, N, K) for N in (384, 1152, 1536) for K in (384, 1536)]
    per_pair = {(BF16, BF16): (1, 2, 3, 4, 6), (E4M3, BF16): (1, 2, 3, 8), (E5M2, BF16): (1, 4, 6, 9)}
    for (ind, outd), forms in per_pair.items():
        for M, N, K in shapes:
            for ncu in NCUS:
                for f in forms:
                    add(ind, outd, M, N, K, FORMS[f], ncu)
    add(E4M3, BF16, 4096, 1536, 256, FORMS[8] + ("fp8_out_only",))
    add(E5M2, BF16, 4096, 1536, 256, FORMS[9] + ("fp8_out_only",))
    add(BF16, BF16, 4096, 1536, 256, FORMS[1], fp8_out_only=1)  # (without fp8_out: ignored)
    # alignment, one flip at a time: vec_ok (ldc, C, ldr, residual), mask_vec_ok (ldmask, relu_mask), the mask prefetch (bias, the
    # byte stride and address of C), warm_b (B's address and byte stride, more than 2 MB of weights)
    flips = [(None, dict(ldc=194)), (None, dict(ldc=196)), (None, dict(ldc=200)), (None, dict(C=ADDR["C"] + 4)), (None, dict(C=ADDR["C"] + 8)),
             (None, dict(B=ADDR["B"] + 64)), (None, dict(B=ADDR["B"] + 16)), (None, dict(ldb=264)), (None, dict(ldb=320)), (None, dict(lda=264)),
             ("residual", dict(ldr=193)), ("residual", dict(ldr=196)), ("residual", dict(residual=ADDR["residual"] + 4)),
             ("residual", dict(residual=ADDR["residual"] + 16)), ("relu_mask", dict(ldmask=193)), ("relu_mask", dict(ldmask=196)),
             ("relu_mask", dict(relu_mask=ADDR["relu_mask"] + 2)), ("relu_mask", dict(relu_mask=ADDR["relu_mask"] + 4)),
             ("relu_mask", dict(relu_mask=ADDR["relu_mask"] + 8)), ("bias", dict(bias=ADDR["bias"] + 4))]       # (the option the flip is about)
    for ind, outd in ((BF16, BF16), (BF16, F32), (F32, F32), (X3, F32), (E4M3, BF16), (E5M2, BF16), (E5M2, F32)):
        for opts in (FORMS[1], FORMS[3], FORMS[7], FORMS[4], FORMS[6], ("relu_mask",), ("sign_bits", "bias")):
            for needs, over in flips:
                if needs is None or needs in opts:
                    add(ind, outd, 256, 192, 256, opts, **over)
    add(BF16, BF16, 256, 8192, 256)                              # 4 MB of weights: no warm-up
    add(BF16, BF16, 256, 4096, 256)                              # exactly 2 MB
    add(E4M3, BF16, 256, 8192, 256)
    # stamped runs: the generic form, no column sums, no fp8 copy
    for ind, outd in ((BF16, BF16), (BF16, F32), (E4M3, BF16), (E5M2, BF16), (X3, F32)):
        for f in (1, 2, 3, 4, 5, 6):
            for N in (128, 192):
                add(ind, outd, 256, N, 256, FORMS[f], stamps=1)
    add(E4M3, BF16, 4096, 1536, 256, FORMS[8], stamps=1)
    # refusals: one per distinct return of dg_gemm_nt
    for k in ("A", "B", "C"):
        add(BF16, BF16, 256, 192, 256, **{k: None})
    for bad in (0, -128):
        add(BF16, BF16, bad, 192, 256)
        add(BF16, BF16, 256, bad, 256, ldc=192)
        add(BF16, BF16, 256, 192, bad, lda=256, ldb=256)
    add(BF16, BF16, 256, 192, 256, in_dtype=9)
    add(BF16, BF16, 256, 192, 256, out_dtype=7)
    add(BF16, BF16, 256, 192, 256, out_dtype=E4M3)
    add(F32, BF16, 256, 192, 256)
    add(X3, BF16, 256, 192, 256)
    add(E4M3, BF16, 256, 192, 256, b_dtype=0)
    add(E4M3, BF16, 256, 192, 256, b_dtype=E5M2)
    add(E5M2, BF16, 256, 192, 256, scale_a=None)
    add(E5M2, BF16, 256, 192, 256, scale_b=None)
    add(BF16, BF16, 256, 192, 256, b_dtype=F32)
    add(BF16, BF16, 256, 192, 256, b_dtype=BF16)
    add(X3, F32, 256, 192, 256, b_dtype=F32)
    add(X3, F32, 256, 192, 256, b_dtype=BF16)
    add(F32, F32, 256, 192, 256, b_dtype=X3)
    for ind, outd in ((BF16, BF16), (F32, F32), (X3, F32), (E4M3, BF16)):
        e = 16 // ESZ[ind]
        add(ind, outd, 256, 192, 256 + e // 2, lda=512, ldb=512)
        add(ind, outd, 256, 192, 256, lda=256 + e // 2)
        add(ind, outd, 256, 192, 256, ldb=256 + e // 2)
        add(ind, outd, 256, 192, 256, A=ADDR["A"] + 8)
        add(ind, outd, 256, 192, 256, B=ADDR["B"] + 8)
        add(ind, outd, 256, 192, 256, lda=256 - e)
        add(ind, outd, 256, 192, 256, ldb=256 - e)
        add(ind, outd, 256, 192, 256, ldc=191)
        add(ind, outd, 256, 192, 256, dropout_p=-0.5)
        add(ind, outd, 256, 192, 256, dropout_p=1.0)
        add(ind, outd, 256, 192, 256, dropout_p=0.5)            # (no rng_state: no dropout)
        add(ind, outd, 256, 192, 256, ("drop",), dropout_p=1.0)
    for ind in (BF16, E4M3, E5M2):
        for o in ("sign_bits", "sign_bits_out"):
            add(ind, BF16, 256, 100, 256, (o,))                  # N % 8
            add(ind, BF16, 256, 192, 256, (o,), sign_bits_bytes=256 * 192 // 8 - 1)
            add(ind, BF16, 256, 192, 256, (o,), sign_bits_bytes=256 * 192 // 8)
            add(ind, BF16, 200, 200, 256, (o,), sign_bits_bytes=2 * 2 * 2048 - 1)
            add(ind, BF16, 200, 200, 256, (o,), sign_bits_bytes=2 * 2 * 2048)
        add(ind, BF16, 256, 192, 256, ("sign_bits", "relu_mask"))
        add(ind, BF16, 256, 192, 256, ("sign_bits_out", "relu_mask"))
        add(ind, BF16, 256, 192, 256, ("bias", "sign_bits", "colsum"))
        add(ind, BF16, 256, 192, 256, ("colsum",))
        add(ind, F32, 256, 192, 256, FORMS[6])
        add(ind, BF16, 256, 192, 256, FORMS[6], colsum_rows=7)
        add(ind, BF16, 256, 192, 256, FORMS[6], colsum_rows=8)
        add(ind, BF16, 256, 192, 256, FORMS[6], colsum_ld=188)
        add(ind, BF16, 256, 192, 256, FORMS[6], colsum_ld=194)
        add(ind, BF16, 256, 192, 256, FORMS[6], colsum_ld=196)
        add(ind, BF16, 256, 192, 256, FORMS[6], colsum_part=ADDR["colsum_part"] + 4)
        add(ind, BF16, 256, 192, 256, FORMS[6], ldc=196)
        add(ind, BF16, 256, 192, 256, FORMS[6], ldc=200)
        add(ind, BF16, 256, 192, 256, FORMS[6], C=ADDR["C"] + 8)
        add(ind, BF16, 4096, 1536, 256, FORMS[6], colsum_rows=127, ncu=256)
        add(ind, BF16, 4096, 1536, 256, FORMS[6], colsum_rows=128, ncu=256)
    for ind, f in ((E4M3, 8), (E5M2, 9), (BF16, 8), (BF16, 9), (E4M3, 9), (E5M2, 8)):
        add(ind, BF16, 4096, 1536, 256, FORMS[f])
        add(ind, F32, 4096, 1536, 256, FORMS[f])
        add(ind, BF16, 4096, 1536, 256, FORMS[f], fp8_out_parts2=None)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], fp8_out_step=None)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], fp8_out_scale_inv=None)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], ld_fp8_out=1528)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], ld_fp8_out=1540)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], ld_fp8_out=1544)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], fp8_out=ADDR["fp8_out"] + 4)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], fp8_out=ADDR["fp8_out"] + 8)
        add(ind, BF16, 4096, 1536, 256, FORMS[f], bias=ADDR["bias"] + 4)
        add(ind, BF16, 4096, 1536, 256, FORMS[f] + ("drop",))
        add(ind, BF16, 4096, 1536, 256, FORMS[f], ldc=1540)
    add(E5M2, BF16, 4096, 1536, 256, ("sign_bits", "fp8_out"))  # the e5m2 copy needs the column sums
    # the late refusal: e4m3 operands with a prefetchable sign_bits input pass every check and have no instance
    add(E4M3, BF16, 256, 192, 256, ("sign_bits",))
    add(E4M3, F32, 256, 128, 256, ("sign_bits", "bias"))
    add(E4M3, BF16, 256, 192, 256, ("sign_bits",), C=ADDR["C"] + 8)           # not prefetchable: the generic form reads the bits
    return out


GRID = _grid()
GRID_SHA = hashlib.sha256("\n".join(c.name for c in GRID).encode()).hexdigest()[:16]

# ---------------------------------------------------------------------------------------------------------------------
# the library's own plan
# ---------------------------------------------------------------------------------------------------------------------
LAUNCH_FIELDS = "grid block K tiles_n n_tiles cs_accum vec_ok mask_vec_ok warm_b drop q8_only"
QUERY_FIELDS = "sign_ok colsum_ok colsum_rows fp8_out_ok sign_bits_bytes"
Plan = collections.namedtuple("Plan", "rc name family out_dtype pf nj epi f8 " + LAUNCH_FIELDS + " bn " + QUERY_FIELDS)
# one golden row: rc, kernel name, then these
Row = collections.namedtuple("Row", "rc name " + LAUNCH_FIELDS + " " + QUERY_FIELDS)
FAMILIES = ("gemm_nt_ws_kernel", "gemm_nt_kernel", "gemm_nt_x3_kernel")


@functools.lru_cache(maxsize=1)
def _lib():
    from drakegpt_amd import _lib as L
    L.lib.dg_debug_nt_plan.argtypes = [C.POINTER(L.GemmNtArgs), C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_char_p)]
    L.lib.dg_debug_nt_plan.restype = C.c_int
    return L


def plan_of(args, ncu=0, stamps=0):
    """what dg_gemm_nt does with these arguments on ``ncu`` compute units (0: the device's, 256 without one)"""
    L = _lib()
    out, name = (C.c_int64 * 24)(), C.c_char_p()
    L.check(L.lib.dg_debug_nt_plan(C.byref(args), ncu, stamps, out, C.byref(name)), "dg_debug_nt_plan")
    v = list(out)
    return Plan(v[0], name.value.decode(), *v[1:18], v[18], *v[19:24])


def plan(case):
    return plan_of(case.args(), case.ncu, case.stamps)


def row_of(p):
    return Row(p.rc, p.name, *[getattr(p, f) for f in (LAUNCH_FIELDS + " " + QUERY_FIELDS).split()])


def parse_name(name):
    """(family, out_dtype, pf, nj, epi, f8) of a wave-specialised instance's name; (family,) of another kernel's"""
    m = re.fullmatch(r"gemm_nt_ws_kernel<(bf16_t|float),(true|false),(\d),(\d),(\d)>", name)
    if m:
        return (0, BF16 if m.group(1) == "bf16_t" else F32, int(m.group(2) == "true"), int(m.group(3)), int(m.group(4)), int(m.group(5)))
    return (FAMILIES.index(name.split("<")[0]),)
