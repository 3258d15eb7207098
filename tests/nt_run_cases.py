"""dg_gemm_nt run on the GPU per planned kernel, tile kind and K-step count: the case table of tests/test_gpu_nt_instances.py, its
operands, memory layouts and fp64 references -- TEST INFRASTRUCTURE (CPU).

tests/nt_cases.py pins WHAT dg_gemm_nt plans (nt_plan against the golden file); this file lists calls that are RUN, one or more
for each of the 74 instances of gemm_nt_ws_kernel and the four register-staged kernels.  A RunCase names the kernel it is meant
for; tests/test_nt_run_cases_host.py holds, from the library's own plan (nt_cases.plan_of, made-up addresses with the
alignment of the views), that every case is what it is named for and that the table reaches every kernel and every class
below for every operand family; the GPU test asserts the same from the real argument struct before it launches it.

Per operand family (bf16, e4m3, e5m2, split bf16 "x3"; the staged kernels where they apply):
  K steps against the four-stage LDS ring: nk = 2, 3, 4, 5, 9 (128-byte steps: 64 bf16, 128 fp8, 32 split-fp32 elements; the
  split form starts at nk = 4); both tile widths (N % 192 == 0: 128 x 192, else 128 x 128); ragged M (200); ragged N with
  N % 8 == 0 (200); N % 8 != 0 with ldc % 4 == 0 (100); odd N with dropout (201 inside ldc = 204; 99 with ldc = 99: the
  per-element dg_keep branch); one tile per workgroup; n_tiles = CU count + a few (some workgroups walk two tiles through one
  continuous stage pipeline, some one: the only shapes that scale with the CU count); the staged kernels at K = 8, 40, 104 (100
  for fp32 operands).
Layout flips, as views into larger allocations (layout()): ldc = N + pad, C one element in, ldr / ldmask odd, residual /
relu_mask / bias four bytes in, lda / ldb wider than K.

Operands come in two kinds: "exact" -- iid integers (A, B in [-4, 4], bias and residual in [-8, 8], a relu_mask that holds 0.0
and -0.0, power-of-two fp8 scales, dropout p = 0.5), so that every value and every partial sum of the kernel is exactly
representable and the output must be BIT-EQUAL to the fp64 reference -- and "randn" (dropout p = 0.25), judged element by element
against a derived envelope."""
import collections
import functools
import zlib

import numpy as np
import torch

import nt_cases as T
from oracle import parity as P
from oracle import rng_ref

F32, BF16, E4M3, E5M2, X3 = T.F32, T.BF16, T.E4M3, T.E5M2, T.X3
FORMS = T.FORMS
TORCH = {F32: torch.float32, BF16: torch.bfloat16, E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2, X3: torch.float32}
FAMILY = {F32: "f32", BF16: "bf16", E4M3: "e4m3", E5M2: "e5m2", X3: "x3"}
KSTEP = {BF16: 64, E4M3: 128, E5M2: 128, X3: 32}         # elements per 128-byte K step of the wave-specialised kernel
NK = (2, 3, 4, 5, 9)
STAGED = {(F32, F32): "gemm_nt_kernel<float,float>", (BF16, F32): "gemm_nt_kernel<bf16_t,float>",
          (BF16, BF16): "gemm_nt_kernel<bf16_t,bf16_t>", (X3, F32): "gemm_nt_x3_kernel"}
FLIPS = ("lda", "ldb", "ldc", "c_off", "ldr", "res_off", "ldmask", "mask_off", "bias_off")
FRONT = 128                                              # elements in front of every view: a guard band that keeps 128-byte alignment
SEED, STEP, SITE = 1234, 3, 5                            # the dropout's rng state
FP8_STEP = 4                                             # even step word: the fp8 copy reads slot 1 of parts2 and writes slot 0
FMAX = {E4M3: 448.0, E5M2: 57344.0}
AMAX_PREV = 112.0                                        # FMAX * 2^j (j = -2 / -9): the copy's scale is the power of two FMAX / 112


class RunCase(collections.namedtuple("RunCase", "name ind outd opts M N K flips kernel want uneven")):
    """one dg_gemm_nt call that is run.  opts: the options present (nt_cases.OPTIONS); flips: ((key, value), ...) of FLIPS;
    kernel: the kernel it is meant for (at 256 CUs: the fp8-copy forms exist on no other count); want: plan fields it is named
    for, ((field, value), ...); uneven: n_tiles = CU count + a few"""
    __slots__ = ()

    @property
    def ws(self):
        return self.kernel.startswith("gemm_nt_ws_kernel")

    @property
    def nk(self):
        return self.K // KSTEP[self.ind] if self.ws else None

    @property
    def fp8(self):
        return self.ind in (E4M3, E5M2)

    @property
    def family(self):
        return ("ws " if self.ws else "staged ") + FAMILY[self.ind]

    def flip(self, key, default=0):
        return dict(self.flips).get(key, default)


def ws_name(ind, outd, N, epi, pf=False):
    return "gemm_nt_ws_kernel<%s,%s,%d,%d,%d>" % ("bf16_t" if outd == BF16 else "float", "true" if pf else "false",
                                                  6 if N % 192 == 0 else 4, epi, {BF16: 0, E4M3: 1, E5M2: 2, X3: 3}[ind])


def run_cases(ncu=256):
    """the table; ``ncu`` enters the "uneven" shapes alone (their M), never a name"""
    out, seen = [], set()

    def add(ind, outd, opts, M, N, K, epi=None, pf=False, uneven=False, **kw):
        flips = tuple((k, kw.pop(k)) for k in FLIPS if k in kw)
        kernel = STAGED[(ind, outd)] if epi is None else ws_name(ind, outd, N, epi, pf)
        shape = f"uneven-x{N}x{K}" if uneven else f"{M}x{N}x{K}"
        name = f"{FAMILY[ind]}>{FAMILY[outd]}/{'+'.join(opts) or 'plain'}/{shape}" + "".join(f"/{k}={v}" for k, v in flips)
        assert name not in seen, name
        seen.add(name)
        if uneven:
            tiles_n = -(-N // (192 if N % 192 == 0 else 128))
            M = 128 * (ncu // tiles_n + 1)
        out.append(RunCase(name, ind, outd, tuple(opts), M, N, K, flips, kernel, tuple(sorted(kw.items())), uneven))

    off0 = {BF16: ("bias", "relu", "relu_mask"), F32: ("relu", "residual")}      # two of the combinations that are no named form
    # ---- every listed instance at both tile widths, two K steps, two tiles on two workgroups
    for N in (128, 192):
        K = 128
        for f in (1, 3, 5, 7):
            add(BF16, BF16, FORMS[f], 256, N, K, f)
            add(BF16, F32, FORMS[f], 256, N, K, f)
        add(BF16, BF16, FORMS[2], 256, N, K, 2)
        add(BF16, BF16, FORMS[4], 256, N, K, 4, pf=True)
        add(BF16, BF16, FORMS[6], 256, N, K, 6, pf=True, cs_accum=0)
        add(BF16, BF16, off0[BF16], 256, N, K, 0)
        add(BF16, F32, off0[F32], 256, N, K, 0)
        add(BF16, BF16, ("sign_bits", "bias"), 256, N, K, 0, pf=True)
        add(BF16, F32, ("sign_bits",), 256, N, K, 0, pf=True)
        K = 256
        for f in (1, 2, 3, 5, 7):
            add(E4M3, BF16, FORMS[f], 256, N, K, f)
        for f in (3, 7):
            add(E4M3, F32, FORMS[f], 256, N, K, f)
        add(E4M3, BF16, ("relu",), 256, N, K, 0)
        add(E4M3, F32, FORMS[1], 256, N, K, 0)                        # fp32 output of forms 1 and 5: no instance, EPI 0
        add(E4M3, F32, FORMS[5], 256, N, K, 0)
        add(E4M3, BF16, ("sign_bits",), 256, N, K, 0, c_off=1, vec_ok=0)      # e4m3 reads sign bits un-prefetched only
        add(E5M2, BF16, FORMS[1], 256, N, K, 1)
        add(E5M2, BF16, FORMS[4], 256, N, K, 4, pf=True)
        add(E5M2, BF16, FORMS[6], 256, N, K, 6, pf=True, cs_accum=0)
        add(E5M2, BF16, FORMS[5], 256, N, K, 0)                       # forward forms on e5m2 operands: EPI 0
        add(E5M2, BF16, FORMS[2], 256, N, K, 0)
        add(E5M2, F32, FORMS[1], 256, N, K, 0)
        add(E5M2, F32, FORMS[4], 256, N, K, 0)                        # prefetchable, fp32 output: EPI 0 without the prefetch
        add(E5M2, BF16, ("sign_bits", "bias"), 256, N, K, 0, pf=True)
        K = 128
        for f in (1, 3, 5, 7):
            add(X3, F32, FORMS[f], 256, N, K, f)
        add(X3, F32, ("relu", "relu_mask"), 256, N, K, 0)
    # ---- K steps 3, 4, 5, 9 (2 above; the split form: 4 above, then 5 and 9): a form without and, where the family has one, a
    # form with the mask prefetch, widths alternating
    ladder = {BF16: ((BF16, FORMS[2], 2), (F32, FORMS[3], 3), (BF16, FORMS[7], 7), (F32, FORMS[1], 1)),
              E4M3: ((BF16, FORMS[2], 2), (F32, FORMS[3], 3), (BF16, FORMS[5], 5), (F32, FORMS[7], 7)),
              E5M2: ((BF16, FORMS[1], 1), (F32, FORMS[4], 0), (BF16, FORMS[5], 0), (BF16, FORMS[1], 1)),
              X3: (None, None, (F32, FORMS[3], 3), (F32, FORMS[7], 7))}
    for ind in (BF16, E4M3, E5M2, X3):
        for i, nk in enumerate(NK[1:]):
            K, N = nk * KSTEP[ind], (192, 128)[i & 1]
            if ladder[ind][i]:
                outd, opts, epi = ladder[ind][i]
                add(ind, outd, opts, 256, N, K, epi)
            if ind in (BF16, E5M2):
                f = (4, 6)[i >> 1]
                add(ind, BF16, FORMS[f], 256, N, K, f, pf=True, **({"cs_accum": 0} if f == 6 else {}))
    # ---- shapes
    for ind in (BF16, E4M3, E5M2, X3):
        K = 2 * KSTEP[ind] if ind != X3 else 128
        lo = BF16 if ind != X3 else F32                               # the family's usual output
        f3 = 3 if ind != E5M2 else 0                                  # (e5m2 operands have no form 3: EPI 0)
        emit = FORMS[2] if ind in (BF16, E4M3) else None
        # ragged M, both widths; ragged N (square tiles only); N % 8 != 0 behind ldc % 4 == 0
        add(ind, lo, emit or FORMS[1], 200, 192, K, 2 if emit else 1)
        add(ind, F32, FORMS[3], 200, 128, K, f3)
        add(ind, lo, emit or FORMS[7], 256, 200, K, 2 if emit else (7 if ind != E5M2 else 0))
        add(ind, F32, FORMS[3], 200, 200, K, f3)
        if ind in (BF16, E5M2):                                       # the prefetch declines the edge tiles one by one
            add(ind, BF16, FORMS[4], 200, 200, K, 4, pf=True)
        add(ind, lo, FORMS[1], 256, 100, K, 1)
        add(ind, F32, FORMS[7], 200, 100, K, 7 if ind != E5M2 else 0)
        # odd N with dropout: whole chunks on the vector path up to the last one (fp32 rows of 204 floats), and nothing aligned
        add(ind, F32, FORMS[3], 256, 201, K, f3, ldc=204, ldr=204)
        add(ind, lo, FORMS[3], 200, 99, K, f3, vec_ok=0)
        # more tiles than workgroups, uneven, through one continuous pipeline
        add(ind, lo, FORMS[1] if ind == X3 else (FORMS[2] if emit else FORMS[6]), 0, 1024, K,
            1 if ind == X3 else (2 if emit else 6), pf=not emit and ind != X3, uneven=True)
    add(BF16, BF16, FORMS[6], 0, 576, 128, 6, pf=True, uneven=True)       # ... on the wide tile, three column blocks: a flush per tile
    add(E4M3, F32, FORMS[3], 0, 384, 256, 3, uneven=True)
    # column sums flushed once per launch (cs_accum): eight workgroups of one column block each
    for ind in (BF16, E5M2):
        add(ind, BF16, FORMS[6], 1024, 128, 2 * KSTEP[ind], 6, pf=True, cs_accum=1)
        add(ind, BF16, FORMS[6], 1024, 192, 3 * KSTEP[ind], 6, pf=True, cs_accum=1)
    # ---- layout flips
    for ind in (BF16, E4M3, E5M2, X3):
        K = 2 * KSTEP[ind] if ind != X3 else 128
        lo = BF16 if ind != X3 else F32
        f7 = 7 if ind != E5M2 else 0
        add(ind, lo, FORMS[1], 256, 192, K, 1, ldc=200, lda=K + 64, ldb=K + 32)
        add(ind, lo, FORMS[1], 200, 128, K, 1, c_off=1, vec_ok=0)
        add(ind, F32, FORMS[7], 256, 192, K, f7, ldr=193, vec_ok=0)
        add(ind, F32, FORMS[7], 256, 128, K, f7, res_off=1, ldc=132, vec_ok=0)
        add(ind, F32, FORMS[5], 256, 192, K, 5 if ind in (BF16, X3) else 0, bias_off=1, ldc=196)
        if ind in (BF16, X3):
            add(ind, lo, ("relu_mask",), 256, 192, K, 0, ldmask=193, mask_vec_ok=0)
            add(ind, lo, ("bias", "relu_mask"), 200, 128, K, 0, mask_off=1, ldc=136, mask_vec_ok=0)
        if ind in (BF16, E5M2):                                       # the un-prefetched reader of the sign bits
            add(ind, BF16, ("sign_bits", "bias"), 256, 192, K, 0, bias_off=1)
            add(ind, BF16, FORMS[4], 256, 128, K, 0, ldc=132)         # 264-byte rows: no whole 16-byte chunks
    # ---- the fp8 copy of the output (256 CUs, 256 whole tiles): both widths, and without the bf16 form
    for M, N in ((8192, 512), (4096, 1536)):
        add(E4M3, BF16, FORMS[8], M, N, 256, 8)
        add(E5M2, BF16, FORMS[9], M, N, 256, 9, pf=True)
    add(E4M3, BF16, FORMS[8] + ("fp8_out_only",), 4096, 1536, 256, 8, ldc=1544)
    add(E5M2, BF16, FORMS[9] + ("fp8_out_only",), 8192, 512, 256, 9, pf=True)
    # ---- the register-staged kernels: one, two and four ragged K steps; every epilogue option behind run-time flags
    for (ind, outd) in STAGED:
        opts = iter((FORMS[3], ("bias", "relu", "relu_mask") if ind != X3 else FORMS[7], ("relu_mask", "residual")))
        for K in (8, 40, 104 if ind == BF16 else 100):
            add(ind, outd, next(opts), 200, 200, K)
        add(ind, outd, FORMS[1], 256, 128, 104)
        add(ind, outd, FORMS[3], 136, 99, 40, vec_ok=0)
    add(F32, F32, ("relu_mask",), 200, 100, 256, ldmask=101, c_off=1, vec_ok=0, mask_vec_ok=0)
    add(BF16, BF16, FORMS[7], 256, 201, 72, ldc=204, ldr=204, lda=80)
    return out


CASE_NAMES = [c.name for c in run_cases(256)]


# ---------------------------------------------------------------------------------------------------------------------
# memory layout: every operand is a view into a larger allocation
# ---------------------------------------------------------------------------------------------------------------------
View = collections.namedtuple("View", "rows cols ld off total")          # elements; ``total``: of the allocation


def _view(rows, cols, ld, off, extra_rows=0):
    return View(rows, cols, ld, FRONT + off, FRONT + off + (rows + extra_rows) * ld + 8)


def layout(case, colsum_rows=0):
    """name -> View of every operand of the case.  C carries three guard rows behind it and ldc - N columns between its rows;
    colsum_part three rows and four columns; the fp8 copy eight columns."""
    M, N, K, f = case.M, case.N, case.K, case.flip
    lay = dict(A=_view(M, K, f("lda", K), 0), B=_view(N, K, f("ldb", K), 0), C=_view(M, N, f("ldc", N), f("c_off"), 3))
    if "bias" in case.opts:
        lay["bias"] = _view(1, N, N, f("bias_off"))
    if "residual" in case.opts:
        lay["residual"] = _view(M, N, f("ldr", N), f("res_off"))
    if "relu_mask" in case.opts:
        # four bytes: two bf16 elements, one fp32 element
        lay["relu_mask"] = _view(M, N, f("ldmask", N), f("mask_off") * (2 if case.ind == BF16 else 1))
    if "colsum" in case.opts:
        lay["colsum_part"] = _view(colsum_rows, N, N + 4, 0, 3)
    if "fp8_out" in case.opts:
        lay["fp8_out"] = _view(M, N, N + 8, 0)
    return lay


ESZ = {"A": None, "B": None, "C": None, "bias": 4, "residual": 4, "relu_mask": None, "colsum_part": 4, "fp8_out": 1}


def host_args(case, ncu=256):
    """dg_gemm_nt_args with made-up addresses of the alignment layout() gives the views (nothing is dereferenced)"""
    lay = layout(case, 1 << 20)
    esz = dict(ESZ, A=T.ESZ[case.ind], B=T.ESZ[case.ind], C=T.ESZ[case.outd], relu_mask=T.ESZ[case.ind])
    over = {k: T.ADDR[k] + v.off * esz[k] for k, v in lay.items()}
    over.update(lda=lay["A"].ld, ldb=lay["B"].ld, ldc=lay["C"].ld)
    for k, ld in (("residual", "ldr"), ("relu_mask", "ldmask"), ("colsum_part", "colsum_ld"), ("fp8_out", "ld_fp8_out")):
        if k in lay:
            over[ld] = lay[k].ld
    if {"sign_bits", "sign_bits_out"} & set(case.opts):
        over["sign_bits_bytes"] = sign_bits_bytes(case.M, case.N)
    return T.Case(case.name, case.ind, case.outd, case.M, case.N, case.K, case.opts, ncu, 0, tuple(sorted(over.items()))).args()


def sign_bits_bytes(M, N):
    return int(T._lib().lib.dg_gemm_nt_sign_bits_bytes(M, N))


def check_plan(case, pl, ncu):
    """the case is what it is named for, by the library's plan ``pl`` of its arguments on ``ncu`` compute units"""
    what = (case.name, pl)
    assert pl.rc == 0 and pl.name == case.kernel, what
    want = dict(vec_ok=1, mask_vec_ok=int("relu_mask" in case.opts), drop=int("drop" in case.opts),
                q8_only=int("fp8_out_only" in case.opts))
    want.update(case.want)
    for k, v in want.items():
        assert getattr(pl, k) == v, (k, v) + what
    if case.ws:
        assert pl.K // 64 == case.nk and pl.K % 64 == 0 and pl.bn == (192 if case.N % 192 == 0 else 128), what
        if case.uneven:
            assert pl.grid == ncu < pl.n_tiles < 2 * ncu and pl.n_tiles - ncu <= 16, what
        else:
            assert pl.n_tiles == pl.grid, what                        # one tile per workgroup
    if "colsum" in case.opts:
        assert pl.colsum_rows == (4 * pl.grid // pl.tiles_n if pl.cs_accum else case.M // 32), what


# ---------------------------------------------------------------------------------------------------------------------
# operands and the fp64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


def _ints(shape, bound, g):
    return torch.randint(-bound, bound + 1, shape, generator=g).float()


def _cast(x, dt):
    return x.float().to(TORCH[dt])


def operands(case, kind):
    """the case's operands on the host, in their storage types.  kind: "exact" | "randn"."""
    M, N, K = case.M, case.N, case.K
    g = _gen(case.name, kind)
    exact = kind == "exact"
    bdt = E4M3 if case.fp8 else case.ind
    if exact:
        d = dict(A=_cast(_ints((M, K), 4, g), case.ind), B=_cast(_ints((N, K), 4, g), bdt))
    else:
        amp = {E4M3: 2.0, E5M2: 10.0}.get(case.ind, 1.0)
        d = dict(A=_cast(torch.randn((M, K), generator=g) * amp, case.ind), B=_cast(torch.randn((N, K), generator=g), bdt))
    if case.fp8:
        d["scale_a"], d["scale_b"] = (torch.tensor([2.0 ** -3]), torch.tensor([2.0 ** -2])) if exact else (torch.tensor([0.01]), torch.tensor([0.02]))
    small = (lambda shape: _ints(shape, 8, g)) if exact else (lambda shape: torch.randn(shape, generator=g))
    if "bias" in case.opts:
        d["bias"] = small((N,))
    if "residual" in case.opts:
        d["residual"] = small((M, N))
    if "relu_mask" in case.opts:
        if exact:
            vals = torch.tensor([-2.0, -1.0, -0.0, 0.0, 1.0, 2.0])
            d["relu_mask"] = _cast(vals[torch.randint(0, 6, (M, N), generator=g)], case.ind)
        else:
            d["relu_mask"] = _cast(torch.randn((M, N), generator=g), case.ind)
    d["p"] = (0.5 if exact else 0.25) if "drop" in case.opts else 0.0
    return d


def mask_operands(M, N):
    """the exact bias + ReLU call whose emitted sign bits feed every consuming case of this shape: bf16 integers, K = 128, and the
    mask it must emit (about half the elements, exact zeros among the dropped)"""
    g = _gen("sign bits", M, N)
    A, B, bias = _ints((M, 128), 4, g).bfloat16(), _ints((N, 128), 4, g).bfloat16(), _ints((N,), 8, g)
    return A, B, bias, (A.double() @ B.double().T + bias.double()) > 0


def scale_of(d):
    return d["scale_a"].double().item() * d["scale_b"].double().item() if "scale_a" in d else 1.0


@functools.lru_cache(maxsize=4)
def keep_mask(p, M, N):
    return torch.from_numpy(rng_ref.keep_mask(SEED, STEP, SITE, p, M * N).reshape(M, N).astype(np.float64))


def reference(case, d, sign_mask=None):
    """P.gemm_nt_epilogue_fp64 of the case's operands (+ acc, mag = |A| |B|^T times the scales, keep_scale: everything that
    multiplies the value in front of the residual)"""
    A, B = d["A"].float().double(), d["B"].float().double()
    ss = scale_of(d)
    keep = keep_mask(d["p"], case.M, case.N) if d["p"] else None
    assert ("sign_bits" in case.opts) == (sign_mask is not None)
    r = P.gemm_nt_epilogue_fp64((A @ B.T) * ss, d.get("bias"), "relu" in case.opts, sign_mask,
                                d["relu_mask"].float() if "relu_mask" in d else None, keep, d["p"], d.get("residual"))
    ks = torch.ones(case.M, case.N, dtype=torch.float64)
    if sign_mask is not None:
        ks = ks * sign_mask.double()
    if "relu_mask" in d:
        ks = ks * (d["relu_mask"].float().double() > 0)
    if keep is not None:
        ks = ks * keep / (1.0 - d["p"])
    r.update(mag=(A.abs() @ B.abs().T) * ss, keep_scale=ks, scale=ss)
    return r


def envelopes(case, d, r):
    """(envelope of the stored value, envelope of the pre-activation) of a randn run: P.gemm_envelope over K products -- the
    split contraction: P.x3_envelope --, evaluated on the operands alone"""
    A, B = d["A"].float(), d["B"].float()
    if case.ind == X3:
        return (P.x3_envelope(A, B, case.K, d.get("bias"), d.get("residual"), r["keep_scale"]),
                P.x3_envelope(A, B, case.K, d.get("bias"), None, torch.ones_like(r["keep_scale"])))
    return (P.gemm_envelope(A, B, case.K, d.get("bias"), d.get("residual"), r["scale"], r["keep_scale"]),
            P.gemm_envelope(A, B, case.K, d.get("bias"), None, r["scale"]))


def exact_conditions(case, d, r):
    """what makes bit equality a fair demand of the exact run: every value is an integer multiple of ``unit`` (the product of
    the fp8 scales) and every sum of magnitudes -- any partial sum the kernel could form, in any order -- stays below 2^24 units;
    for fp8 every 128-term K-step sum stays below 2^13, where the instruction's adder keeps every bit
    (tests/test_gpu_tn_instances.py); column sums likewise.  Returns the largest of these in units."""
    unit = r["scale"]
    top = r["mag"].max().item() / unit
    if "bias" in d:
        top += 8 / unit
    if d["p"]:
        top *= 2
    if "residual" in d:
        top += 8 / unit
    assert top < 2 ** 24, (case.name, top)
    assert bool(((r["out"] / unit).round() == r["out"] / unit).all()), case.name
    if case.fp8:
        A, B = d["A"].float().abs(), d["B"].float().abs()
        step = max((A[:, k:k + 128] @ B[:, k:k + 128].T).max().item() for k in range(0, case.K, 128))
        assert step < 2 ** 13, (case.name, step)
    if "colsum" in case.opts:
        cs = r["out"].abs().sum(0).max().item() / unit
        assert cs < 2 ** 24, (case.name, cs)
        top = max(top, cs)
    return top
