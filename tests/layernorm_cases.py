"""csrc/layernorm.hip: its host dispatch restated in Python, and the case tables of tests/test_gpu_layernorm.py -- TEST
INFRASTRUCTURE (CPU).

Three things pick the template instance that an entry point launches: the width class nk = ceil(C / 256) (float4 slices per
lane on the vector path), whether the vector path applies (C % 4 == 0, C <= 2048, every operand 16-byte aligned) and the dtypes of dy, g and the
residual-gradient stream.  ``instance`` follows ``dg_layernorm_fwd``, ``dg_layernorm_fwd_fp8`` and ``ln_bwd_launch`` line by
line and names the instance (or "rejected"); tests/test_layernorm_cases_host.py holds the tables below against the list of
instances written out from the launches of the kernel file: every instance needs a case whose slices are all full and, where its width
class allows, one whose last slice is partially filled.

The operands and the fp64 reference are computed once per width for ROWS_MAX rows and shared: LayerNorm is row-local, so a
case with M rows runs on the first M rows and is compared with the first M rows of the reference (the keep mask of element
(m, c) is a function of m * C + c alone); only the column sums depend on M, and they are summed per case from stored terms.
Nothing returned from the caches is modified."""
import collections
import functools

import torch

from oracle import parity as P
from oracle import rng_ref

F32, BF16 = "f32", "bf16"
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
LN_MAXV_CAP = 8
ROWS_MAX = 517
SEED, STEP, SITE = 4321, 3, 9
ENTRIES = ("fwd", "fwd_fp8", "bwd", "bwd_fused", "bwd_fused_fp8")
FP8_AMAX_PARTS = 256


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch
# ---------------------------------------------------------------------------------------------------------------------
def width_class(C):
    return (C + 255) // 256


WIDTH_TABLE = {1: (1, 1024), 2: (2, 1024), 3: (3, 512), 4: (4, 512)}       # nk -> (LN_MAXV, backward threads); above: (8, 256)


def width(C):
    return WIDTH_TABLE.get(max(width_class(C), 1), (8, 256))


def instance(entry, C, aligned=True, dy_dtype=F32, g_dtype=F32, stream_dtype=F32, fp8=False, out_dtype=F32):
    """the template instance ``entry`` launches for width C, or "rejected".  aligned: every operand on a 16-byte boundary.
    out_dtype: y of the forward.  fp8: the fused backward's e5m2 form (the same instance with a uniform run-time branch)."""
    assert entry in ENTRIES, entry
    vec = C % 4 == 0 and C <= 64 * 4 * LN_MAXV_CAP and aligned
    nk = width_class(C)
    if entry == "fwd":
        if not vec:
            return f"ln_fwd_scalar_kernel<{out_dtype}>"
        return f"ln_fwd_kernel<{out_dtype},{width(C)[0]}>"
    if entry == "fwd_fp8":
        if C % 4 or C > 64 * 4 * 4 or not aligned:
            return "rejected"
        return f"ln_fwd_fp8_kernel<{width(C)[0]}>"
    fp8 = fp8 or entry == "bwd_fused_fp8"
    if entry == "bwd":
        if fp8 or stream_dtype != F32:
            return "rejected"
        fuse = 0
    else:
        if fp8 and g_dtype != BF16:
            return "rejected"
        fuse = 1 if g_dtype == BF16 else 2
    if fuse and (not vec or nk > 4):
        return "rejected"
    if dy_dtype == BF16 and not vec:
        return "rejected"
    if stream_dtype == BF16 and (not vec or fuse != 1 or dy_dtype != BF16):
        return "rejected"
    k, nt = width(C)
    if 2 * (nt // 64) * C * 4 > 64 * 1024:
        return "rejected"
    if not vec:
        return f"ln_bwd_scalar_kernel<{nt}>"
    if stream_dtype == BF16:            # the last argument: rows in flight ahead of the one being computed
        return f"ln_bwd_kernel<bf16,{k},{nt},1,bf16,{1 if k == 2 else 2}>"
    return f"ln_bwd_kernel<{dy_dtype},{k},{nt},{fuse},f32,0>"


def slices(C):
    """(all slices of the instance's width class full, last slice partially filled) for a vector-path width; the scalar path
    walks the row 64 columns at a time, and the same two words describe its last round"""
    return C % 256 == 0 and (C <= 1024 or C == 2048), (C // 4) % 64 != 0


def scalar_slices(C):
    return C % 64 == 0, C % 64 != 0


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "entry C misaligned dy g stream out p dresid gbias rows")):
    """misaligned: the operand that sits 4 bytes past a 16-byte boundary (None: all aligned); dy / g / stream / out: dtype names;
    dresid / gbias: given or None; rows: the M (forward) or (M, n_partials) (backward) values the case runs at"""
    __slots__ = ()

    @property
    def instance(self):
        return instance(self.entry, self.C, self.misaligned is None, self.dy, self.g or F32, self.stream, self.entry == "bwd_fused_fp8", self.out)

    @property
    def id(self):
        s = f"{self.entry}-C{self.C}"
        if self.entry in ("fwd", "fwd_fp8"):
            s += f"-{self.out}"
        else:
            s += f"-dy_{self.dy}" + (f"-g_{self.g}" if self.g else "") + ("-stream_bf16" if self.stream == BF16 else "")
            s += (f"-p{self.p:g}" if self.entry != "bwd" else "") + ("-dresid" if self.dresid else "") + ("-gbias" if self.gbias else "")
        return s + (f"-{self.misaligned}_plus4" if self.misaligned else "")


def case(entry, C, misaligned=None, dy=F32, g=None, stream=F32, out=F32, p=0.0, dresid=False, gbias=False, rows=None):
    return Case(entry, C, misaligned, dy, g, stream, out, p, dresid, gbias, rows)


ROWS_FWD = (1, 2, 7, 9, 517)                 # a workgroup covers 8 rows, a wave 2: a lone wave with one row, a second workgroup with one row, odd M
# rows_per = ceil(M / G) = 1, 1, 3, 18, 33 against NW = 16 / 8 / 4 waves: workgroups without rows (3 of 4, 19 of 24, 2 of 16), fewer
# rows than waves, one to three rounds per wave, ragged last rounds and a ragged last chunk (517 = 15 * 33 + 22)
ROWS_BWD = ((1, 4), (5, 24), (40, 16), (70, 4), (517, 16))
# the prefetching instance keeps one (nk = 2) or two rows per wave in flight: rows_per = 1, 5, 9, 17, 18, 33 against NW = 16 / 8
ROWS_STREAM = ((3, 4), (17, 4), (33, 4), (65, 4), (70, 4), (130, 4))
ROWS_FP8_BWD = ((100, FP8_AMAX_PARTS), (300, FP8_AMAX_PARTS))     # rows_per = 1 / 2: 156 / 106 workgroups without rows
ROWS_FP8_FWD = (1, 7, 9, 100)

SCALAR_WIDTHS = (1, 3, 30, 63, 65, 101, 510, 1001, 2046)           # C % 4 != 0; all three thread counts of the backward
# each the smallest that can go wrong in its class: one live lane, a ragged lane count, nk = 1 .. 4 full and one float4 more,
# LN_MAXV = 8 with three / two / one empty slices, one lane short of full, full
VECTOR_WIDTHS = (4, 100, 256, 260, 512, 516, 768, 772, 1020, 1024, 1028, 1280, 1600, 2044, 2048)
FUSED_WIDTHS = tuple(C for C in VECTOR_WIDTHS if C <= 1024)
STREAM_WIDTHS = (100, 256, 384, 512, 516, 768, 772, 1024)
FP8_FWD_WIDTHS = (4, 100, 256, 260, 512, 516, 768, 772, 1024)
FP8_BWD_WIDTHS = (260, 1024)

FWD_CASES = [case("fwd", C, out=o, rows=ROWS_FWD) for C in SCALAR_WIDTHS + (4096,) + VECTOR_WIDTHS for o in (F32, BF16)]
FWD_CASES += [case("fwd", 384, misaligned=m, out=o, rows=ROWS_FWD) for m in ("x", "gamma") for o in (F32, BF16)]

BWD_CASES = [case("bwd", C, dresid=C not in (30, 1001), rows=ROWS_BWD) for C in SCALAR_WIDTHS]
BWD_CASES += [case("bwd", 384, misaligned=m, dresid=True, rows=ROWS_BWD) for m in ("x", "gamma", "dy", "dx")]
BWD_CASES += [case("bwd", C, misaligned="x", dresid=True, rows=ROWS_BWD) for C in (768, 2048)]      # whole 64-column rounds at 512 / 256 threads
BWD_CASES += [case("bwd", C, dy=d, dresid=C not in (260, 1600), rows=ROWS_BWD) for C in VECTOR_WIDTHS for d in (F32, BF16)]

# the options of the fused form, crossed thinly: every value of g / dy dtype, p, dresid and gbias_part at every width, hence at
# a full and at a ragged width of every class.  The last two mix the dtypes (instances the entry point also launches).
FUSED_OPTIONS = (dict(dy=F32, g=F32, p=0.2, dresid=True, gbias=True), dict(dy=BF16, g=BF16, p=0.0, dresid=False, gbias=False),
                 dict(dy=BF16, g=BF16, p=0.2, dresid=True, gbias=True), dict(dy=F32, g=F32, p=0.0, dresid=False, gbias=True),
                 dict(dy=F32, g=BF16, p=0.2, dresid=False, gbias=True), dict(dy=BF16, g=F32, p=0.0, dresid=True, gbias=False))
FUSED_CASES = [case("bwd_fused", C, rows=ROWS_BWD, **o) for C in FUSED_WIDTHS for o in FUSED_OPTIONS]

STREAM_CASES = [case("bwd_fused", C, dy=BF16, g=BF16, stream=BF16, p=p, dresid=r, gbias=r, rows=ROWS_STREAM)
                for C in STREAM_WIDTHS for r in (True, False) for p in (0.0, 0.2)]

FP8_BWD_CASES = [case("bwd_fused_fp8", C, dy=BF16, g=BF16, stream=s, p=0.2, dresid=True, gbias=True, rows=ROWS_FP8_BWD)
                 for C in FP8_BWD_WIDTHS for s in (BF16, F32)]
FP8_FWD_CASES = [case("fwd_fp8", C, out=BF16, rows=ROWS_FP8_FWD) for C in FP8_FWD_WIDTHS]

ALL_CASES = FWD_CASES + BWD_CASES + FUSED_CASES + STREAM_CASES + FP8_BWD_CASES + FP8_FWD_CASES

# a RuntimeError before any launch.  (entry, C, misaligned operand, dy, g, stream)
REJECTED = [("bwd", 30, None, BF16, None, F32), ("bwd", 384, "dy", BF16, None, F32),
            ("bwd_fused", 30, None, F32, F32, F32), ("bwd_fused", 1028, None, F32, F32, F32), ("bwd_fused", 384, "g", F32, F32, F32),
            ("bwd", 2050, None, F32, None, F32), ("bwd", 4096, None, F32, None, F32),
            ("bwd_fused", 384, None, F32, BF16, BF16)]


# ---------------------------------------------------------------------------------------------------------------------
# operands and references, once per width
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def operands(C):
    """x ~ 2 N + 0.5 (a mean that does not vanish), gamma, beta, dy, dresid ~ N: fp32 host tensors for ROWS_MAX rows"""
    g = torch.Generator().manual_seed(1000 + C)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(x=rn(ROWS_MAX, C) * 2 + 0.5, w=rn(C), b=rn(C), dy=rn(ROWS_MAX, C), dres=rn(ROWS_MAX, C))


@functools.lru_cache(maxsize=4)
def keep_scale(C, p):
    """keep (fp64 {0, 1} [ROWS_MAX, C]) of the dropout site the fused cases use; None at p = 0"""
    if p == 0:
        return None
    return torch.from_numpy(rng_ref.keep_mask(SEED, STEP, SITE, p, ROWS_MAX * C).reshape(ROWS_MAX, C)).double()


@functools.lru_cache(maxsize=4)
def forward_reference(C):
    """(fp64 reference, fp32 model) of the forward: dicts y / mean / rstd / xhat, [ROWS_MAX, ...]"""
    op = operands(C)
    y, mean, std, xhat = P.layernorm_fp64(op["x"], op["w"], op["b"])
    return dict(y=y, mean=mean, std=std, rstd=1.0 / std, xhat=xhat), P.layernorm_model(op["x"], op["w"], op["b"])


@functools.lru_cache(maxsize=4)
def backward_reference(C, dy_dtype, stream_dtype, dresid, p):
    """(fp64 reference, fp32 model) of the backward on the operands as the kernel receives them (dy / dresid rounded to their
    dtype first).  The reference's dx is autograd's through torch.nn.functional.layer_norm in double; its column-sum terms come
    from layernorm_fp64's xhat.  Both: dx, g, dgamma_terms, dbeta_terms, gbias_terms [ROWS_MAX, C]."""
    op = operands(C)
    dy = op["dy"].to(TORCH[dy_dtype]).double()
    dres = op["dres"].to(TORCH[stream_dtype]).double() if dresid else None
    keep = keep_scale(C, p)
    xd = op["x"].double().requires_grad_(True)
    torch.nn.functional.layer_norm(xd, (C,), op["w"].double(), op["b"].double(), 1e-5).backward(dy)
    dx = xd.grad if dres is None else xd.grad + dres
    g = dx if keep is None else dx * keep / (1.0 - p)
    xhat = forward_reference(C)[0]["xhat"]
    ref = dict(dx=dx, g=g, dgamma_terms=dy * xhat, dbeta_terms=dy, gbias_terms=g)
    return ref, P.layernorm_model(op["x"], op["w"], op["b"], dy, dres, keep, p)
