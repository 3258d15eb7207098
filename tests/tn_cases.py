"""The dW (TN) GEMMs of csrc/gemm.hip -- dg_gemm_tn (four kernels, split-K slabs) and dg_gemm_tn_grouped (a bf16 and an fp8
body, calls of more problems than one launch holds): the case tables of tests/test_gpu_tn_instances.py, their operands and
fp64 references -- TEST INFRASTRUCTURE (CPU).

Nothing in the suite can observe WHICH kernel, split map or split mode a launch took.  The library therefore reports its own
launch plan through two diagnostic entries (dg_debug_tn_plan, dg_debug_tn_grouped_plan: the host functions the launch paths
themselves call, pure host code that runs without a GPU), and the class of every case below is read from that plan -- there
is no second copy of the dispatch here.  The only restatement is ``tn_work`` (with ``xcd_remap``), the device-side map from a
workgroup to its (tile, split): tests/test_tn_cases_host.py holds it to be a bijection, holds the kernel names the plan can
return against the hipLaunchKernelGGL targets read from the source text, and holds ``CASES(ncu)`` to reach every class listed
in ``MAT_CLASSES`` / ``GROUP_CLASSES`` for three CU counts.  The GPU tests then assert, with the CU count of the device they run
on, that each case is the case it is named for.

Classes of a per-matrix launch: (kernel, map, nk) with
  kernel  "ws" | "bf16" | "f32" | "x3"             gemm_tn_<kernel>_kernel
  map     "share8" / "share4" / "share2"           1-D grid, S = 1 / 2 / 4: a split owns 8 / S XCDs (padding workgroups when the
                                                   tile count is no multiple of that share)
          "groups1" / "groups2"                    1-D grid, S = 8 / 16: S / 8 splits per XCD
          "grid2d"                                 every other S: 2-D grid with dg_xcd_remap over the tiles
  nk      (K steps of split 0 -- 5 stands for "5 or more" --, last split "full" | "short" | "empty", some split ragged)
          with 64-row steps for the bf16 kernels and 32-row steps for f32 / x3.
Classes of a grouped call: (body, "single" | "multi", the sorted split modes of its launches).  Mode 3 (only the leftover tiles
of the last round are cut) needs more tiles than CUs; tests/test_gpu_ops.py runs it with 384 tiles and it has no case here."""
import collections
import ctypes as C
import functools

import torch

from oracle import parity as P

BF16, F32, X3 = "bf16", "f32", "x3"
DT_CODE = {F32: 0, BF16: 1, X3: 4}
FP8_CODE = 3
TORCH = {BF16: torch.bfloat16, F32: torch.float32, X3: torch.float32}
STEP_ROWS = {"ws": 64, "bf16": 64, "f32": 32, "x3": 32}
CHUNK = {BF16: 8, F32: 4, X3: 4}               # elements per 16-byte chunk
PART_BYTES = 8 * 16384                         # partials per 256 x 128 tile of the grouped kernel
MAX_GROUP = {False: 64, True: 48}              # problems per launch: bf16, fp8
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------------
# the library's own plan
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _lib():
    from drakegpt_amd import _lib as L
    lib = L.lib
    lib.dg_debug_tn_plan.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int), C.POINTER(C.c_char_p)]
    lib.dg_debug_tn_plan.restype = C.c_int
    lib.dg_debug_tn_grouped_plan.argtypes = [C.POINTER(L.TnProblem), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int]
    lib.dg_debug_tn_grouped_plan.restype = C.c_int
    return L


Plan = collections.namedtuple("Plan", "kernel xcd_map grid_x grid_y block r_per_split tiles_q n_tiles")
Launch = collections.namedtuple("Launch", "first count tiles tiles_pad splits grid flag_offset ws_need")


def plan(R, Pn, Q, S, dtype, ncu=0):
    """what dg_gemm_tn launches for these arguments on ``ncu`` compute units (0: the device's); kernel by name"""
    L = _lib()
    out, name = (C.c_int * 8)(), C.c_char_p()
    L.check(L.lib.dg_debug_tn_plan(R, Pn, Q, S, DT_CODE[dtype], ncu, out, C.byref(name)), "dg_debug_tn_plan")
    return Plan(name.value.decode(), *list(out)[1:])


def problem_array(shapes):
    """dg_tn_problem array carrying R, P, Q only (what the plan and the size function read)"""
    L = _lib()
    arr = (L.TnProblem * len(shapes))()
    for t, (R, Pn, Q) in zip(arr, shapes):
        t.R, t.P, t.Q = R, Pn, Q
    return arr


def grouped_plan(shapes, f8, with_ws, ncu=0):
    """the launches of dg_gemm_tn_grouped on problems of these (R, P, Q)"""
    L = _lib()
    rows = (C.c_int64 * (8 * (len(shapes) // 48 + 2)))()
    n = L.lib.dg_debug_tn_grouped_plan(problem_array(shapes), len(shapes), FP8_CODE if f8 else DT_CODE[BF16], int(with_ws), ncu, rows, len(rows) // 8)
    assert 0 < n <= len(rows) // 8, n
    return [Launch(*rows[8 * i:8 * i + 8]) for i in range(n)]


def workspace_bytes(shapes):
    return int(_lib().lib.dg_gemm_tn_grouped_workspace_bytes(problem_array(shapes), len(shapes)))


def group_tiles(Pn, Q):
    """256 x 128 tiles of a grouped problem"""
    return -(-Pn // 256) * -(-Q // 128)


# ---------------------------------------------------------------------------------------------------------------------
# the device-side work map (the one restatement)
# ---------------------------------------------------------------------------------------------------------------------
def xcd_remap(orig, nwg):
    """dg_xcd_remap (common.h)"""
    q, r, xcd = nwg // 8, nwg % 8, orig % 8
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + orig // 8


def tn_work(bx, by, n_tiles, S, xcd_map):
    """tn_work: (tile, split) of workgroup (bx, by); tile >= n_tiles is a padding workgroup"""
    if not xcd_map:
        return xcd_remap(bx, n_tiles), by
    x, rest = bx & 7, bx >> 3
    if S >= 8:
        g = S >> 3
        return rest // g, x + 8 * (rest % g)
    share = 8 // S
    return rest * share + x // S, x % S


# ---------------------------------------------------------------------------------------------------------------------
# classes
# ---------------------------------------------------------------------------------------------------------------------
def slab_rows(R, S, r_per_split):
    """[lo, hi) of the contraction rows each split's slab sums"""
    return [(min(R, s * r_per_split), min(R, (s + 1) * r_per_split)) for s in range(S)]


def classify(R, Pn, Q, S, dtype, ncu=0):
    pl = plan(R, Pn, Q, S, dtype, ncu)
    kernel = pl.kernel[len("gemm_tn_"):-len("_kernel")]
    if not pl.xcd_map:
        mp = "grid2d"
    else:
        mp = f"groups{S // 8}" if S >= 8 else f"share{8 // S}"
    br = STEP_ROWS[kernel]
    rows = [hi - lo for lo, hi in slab_rows(R, S, pl.r_per_split)]
    last = "empty" if rows[-1] == 0 else ("short" if rows[-1] < rows[0] else "full")
    return kernel, mp, (min(-(-rows[0] // br), 5), last, any(r % br for r in rows))


MAP_OF = {1: "share8", 2: "share4", 3: "grid2d", 4: "share2", 5: "grid2d", 6: "grid2d", 7: "grid2d", 8: "groups1", 9: "grid2d", 16: "groups2"}
KINDS = ("ws", "bf16", "f32", "x3")
DTYPE_OF = {"ws": BF16, "bf16": BF16, "f32": F32, "x3": X3}
EDGE_SHAPES = ((128, 128), (200, 72), (136, 264), (48, 40), (384, 70))
LAYOUTS = ("plain", "padded", "out+1", "ldo4")

# what CASES(ncu) must reach for every ncu: every kernel under every map; the K-step ladder of the ws kernel and its short and
# empty last splits; one, two and three ragged steps and an empty split on the staged kernels
MAT_CLASSES = {(k, m) for k in KINDS for m in ("share8", "share4", "share2", "grid2d", "groups1", "groups2")}
NK_CLASSES = {("ws", (n, "full", False)) for n in (1, 2, 3, 4, 5)} | {("ws", (2, "short", False)), ("ws", (1, "empty", False))}
NK_CLASSES |= {(k, (n, "full", True)) for k in ("bf16", "f32", "x3") for n in (1, 2, 3)} | {(k, (1, "empty", True)) for k in ("bf16", "f32", "x3")}


class Mat(collections.namedtuple("Mat", "name kind R P Q S layout want_map want_nk")):
    """one dg_gemm_tn launch.  kind: the kernel it is meant to reach; want_map / want_nk: the class it is named for (None: not
    what the case is about)"""
    __slots__ = ()

    @property
    def dtype(self):
        return DTYPE_OF[self.kind]

    def check_class(self, ncu=0):
        kernel, mp, nk = classify(self.R, self.P, self.Q, self.S, self.dtype, ncu)
        assert kernel == self.kind, (self.name, kernel)
        assert self.want_map is None or mp == self.want_map, (self.name, mp)
        assert self.want_nk is None or nk == self.want_nk, (self.name, nk)
        return kernel, mp, nk


def mat_cases(ncu):
    """ncu only enters the one case whose class depends on it: the staged bf16 kernel reached because the launch is more
    than one round of workgroups (36 tiles x S > ncu).  Every other bf16 "ws" case has at most 63 workgroups, one round on any
    CU count >= 64 (the other counts of the host test, 304 and 64, are arbitrary: one larger than the MI355X's 256 that is no
    multiple of 36, one at the lower edge)."""
    out = []

    def add(name, kind, R, Pn, Q, S, layout="plain", want_map=None, want_nk=None):
        assert R <= 2240 and -(-Pn // 128) * -(-Q // 128) <= 9 or name == "two-rounds", name
        out.append(Mat(name, kind, R, Pn, Q, S, layout, want_map, want_nk))

    # K steps per split
    for n in (1, 2, 3, 4, 5):
        add(f"ws-{n}-steps", "ws", 64 * n, 128, 128, 1, want_map="share8", want_nk=(n, "full", False))
    add("ws-short-last-split", "ws", 192, 128, 128, 2, want_map="share4", want_nk=(2, "short", False))
    add("ws-empty-last-split", "ws", 128, 128, 128, 3, want_map="grid2d", want_nk=(1, "empty", False))
    for kind, rs in (("bf16", (40, 100, 130, 70)), ("f32", (20, 50, 65, 35)), ("x3", (20, 50, 65, 35))):
        for n, R in enumerate(rs[:3], 1):
            add(f"{kind}-{n}-ragged-steps", kind, R, 128, 128, 1, want_map="share8", want_nk=(n, "full", True))
        add(f"{kind}-empty-split", kind, rs[3], 128, 128, 3, want_map="grid2d", want_nk=(1, "empty", True))
    # split maps: 3 tiles (no multiple of the share 8 / S of S = 1, 2, 4), 9 tiles on the 2-D grid; every split has rows of its own
    for kind in KINDS:
        for S in (1, 2, 4, 5, 6, 7, 8, 16):
            Pn, Q = (384, 384) if S in (5, 6, 7) else (384, 128)
            R = {"ws": 1024 if S == 16 else 128 * S, "bf16": 64 * S - 24, "f32": 32 * S - 12, "x3": 32 * S - 12}[kind]
            add(f"{kind}-map-S{S}", kind, R, Pn, Q, S, want_map=MAP_OF[S])
    # the production route to the staged bf16 kernel: whole 64-row steps, more workgroups than CUs
    S = ncu // 36 + 1
    add("two-rounds", "bf16", 128 * S, 768, 768, S, want_map=MAP_OF.get(S))
    # edges, two slabs each
    for kind, R in (("ws", 128), ("bf16", 100), ("f32", 72), ("x3", 72)):
        for Pn, Q in EDGE_SHAPES:
            for layout in ("padded", "out+1") + (("ldo4",) if Q % 4 else ()):
                add(f"{kind}-{Pn}x{Q}-{layout}", kind, R, Pn, Q, 2, layout, want_map="share4")
    return out


class Group(collections.namedtuple("Group", "name f8 R shapes want")):
    """one dg_gemm_tn_grouped call: problems of (P, Q) ``shapes`` over R rows.  want: per launch (tiles, cut) with cut True / False /
    None (depends on the CU count: not asserted) when a workspace is passed"""
    __slots__ = ()

    @property
    def rpq(self):
        return [(self.R, Pn, Q) for Pn, Q in self.shapes]

    def check_class(self, ncu=0):
        """(launches with a workspace, launches without one), each asserted against ``want``"""
        cut, whole = grouped_plan(self.rpq, self.f8, True, ncu), grouped_plan(self.rpq, self.f8, False, ncu)
        assert [l.tiles for l in cut] == [t for t, _ in self.want] == [l.tiles for l in whole], (self.name, cut)
        assert all(l.splits == 1 and l.ws_need == 0 for l in whole), (self.name, whole)
        for l, (_, c) in zip(cut, self.want):
            assert c is None or l.splits == (2 if c else 1), (self.name, l)
        return cut, whole

    def group_class(self, ncu=0):
        cut = grouped_plan(self.rpq, self.f8, True, ncu)
        return ("fp8" if self.f8 else "bf16", "multi" if len(cut) > 1 else "single", tuple(sorted({l.splits for l in cut})))


ONE_TILE = ((256, 128), (200, 72), (80, 128), (136, 104), (48, 40), (256, 70))
FP8_SINGLE_SHAPES = ((80, 384), (330, 100), (100, 330), (264, 520))
# what CASES(ncu) must reach for every ncu: the fp8 body whole and in halves, and for both bodies a call of several launches of
# which at least one is cut (which of them are depends on the CU count, see group_cases)
GROUP_CLASSES = {("fp8", "single", (1,)), ("fp8", "single", (2,))}
MULTI_BODIES = ("bf16", "fp8")


def group_cases(ncu):
    """A launch of T tiles is cut in two K halves when 2 * roundup(T, 8) <= ncu (and it has two K steps or more): the small second
    launches below are cut on every CU count, the first ones of 48 / 64 one-tile problems from 96 / 128 CUs on (None)."""
    out = []
    ones = lambda n: [ONE_TILE[i % len(ONE_TILE)] for i in range(n)]
    big = lambda t: None if 2 * t > ncu else True
    for R in (128, 256, 384, 512):
        for Pn, Q in FP8_SINGLE_SHAPES:
            out.append(Group(f"fp8-{Pn}x{Q}-R{R}", True, R, [(Pn, Q)], [(group_tiles(Pn, Q), R >= 256)]))
    out.append(Group("bf16-70x1", False, 128, ones(70), [(64, big(64)), (6, True)]))
    out.append(Group("fp8-52x1", True, 256, ones(52), [(48, big(48)), (4, True)]))
    out.append(Group("bf16-64x1+8x12", False, 128, ones(64) + [(768, 512)] * 8, [(64, big(64)), (96, big(96))]))
    out.append(Group("fp8-48x1+8x10", True, 256, ones(48) + [(512, 640)] * 8, [(48, big(48)), (80, big(80))]))
    out.append(Group("fp8-48x1+48x2+4x1", True, 256, ones(48) + [(512, 128), (256, 256)] * 24 + ones(4), [(48, big(48)), (96, big(96)), (4, True)]))
    return out


def CASES(ncu):
    return mat_cases(ncu), group_cases(ncu)


# ---------------------------------------------------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------------------------------------------------
def _ru(x, m):
    return -(-x // m) * m


Layout = collections.namedtuple("Layout", "lda ldb ldo offset slab stride total")


def layout(case):
    """leading dimensions, the offset of ``out`` in its buffer (floats), the extent of a slab, the slab stride and the buffer size"""
    ch, Pn, Q = CHUNK[case.dtype], case.P, case.Q
    lda, ldb, ldo, off = _ru(Pn, ch), _ru(Q, ch), Q, 0
    if case.layout == "padded":
        lda, ldb, ldo = lda + ch, ldb + ch, Q + 5
    elif case.layout == "out+1":
        off = 1
    elif case.layout == "ldo4":
        assert Q % 4
        ldo = _ru(Q, 4)
    slab = (Pn - 1) * ldo + Q
    stride = {"padded": slab + 37, "ldo4": Pn * ldo}.get(case.layout, slab)
    if case.layout == "ldo4":
        assert ldo % 4 == 0 and stride % 4 == 0
    return Layout(lda, ldb, ldo, off, slab, stride, off + (case.S - 1) * stride + slab + 19)


@functools.lru_cache(maxsize=8)
def _draw(kind, R, width, seed):
    """[R, width] fp32: "exact" iid integers in [-4, 4], "randn" N(0, 1).  Never modified."""
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        return torch.randint(-4, 5, (R, width), generator=g).float()
    return torch.randn(R, width, generator=g)


def mat_operands(case, kind):
    """(A [R, lda], B [R, ldb]) in the case's dtype, NaN behind columns P / Q; and the same values [R, P], [R, Q] in fp64"""
    lay, dt = layout(case), TORCH[case.dtype]
    A = torch.full((case.R, lay.lda), NAN).to(dt)
    B = torch.full((case.R, lay.ldb), NAN).to(dt)
    A[:, :case.P] = _draw(kind, case.R, 768, 1)[:, :case.P].to(dt)
    B[:, :case.Q] = _draw(kind, case.R, 768, 2)[:, :case.Q].to(dt)
    return A, B, A[:, :case.P].double(), B[:, :case.Q].double()


def slab_references(Ad, Bd, rows):
    """per slab: the fp64 product over its own rows, sum |a||b| over them, its row count"""
    return [(Ad[lo:hi].T @ Bd[lo:hi], Ad[lo:hi].abs().T @ Bd[lo:hi].abs(), hi - lo) for lo, hi in rows]


def slab_envelope(mag, rows, fp32):
    """fp32 accumulation of one slab: bf16 products are exact in fp32, so K = rows roundings of a running sum bounded by
    sum |a||b|; an fp32 product is rounded once before it is added, K = 2 rows (oracle/parity.py, gemm_envelope)"""
    return mag * ((2 if fp32 else 1) * rows * 2.0 ** -24)


def sum_envelope(refs, fp32):
    """dg_reduce_partials adds the S slabs in fp32, one at a time: S - 1 more roundings of a running sum bounded by the sum of
    the slabs' own bounds sum |a||b| (1 + their envelope), on top of every slab's envelope -- S roundings to have room"""
    S = len(refs)
    return sum(slab_envelope(mag, rows, fp32) + mag * (S * 2.0 ** -24) for _, mag, rows in refs)


def fp8_values(kind, R, Pn, Q, seed):
    """(A [R, P] e5m2, B [R, Q] e4m3, scale_a, scale_b): "exact" integers in [-4, 4] / [-8, 8] (both exact in their format; a
    128-row K step sums to at most 128 * 32 = 2^12) with power-of-two scales, "randn" as tests/test_gpu_fp8.py draws them"""
    g = torch.Generator().manual_seed(seed)
    if kind == "exact":
        A, B = torch.randint(-4, 5, (R, Pn), generator=g).float(), torch.randint(-8, 9, (R, Q), generator=g).float()
        sa, sb = 0.5, 4.0
    else:
        A, B = torch.randn(R, Pn, generator=g) * 3.0, torch.randn(R, Q, generator=g)
        sa, sb = 0.37, 1.9
    return A.to(torch.float8_e5m2), B.to(torch.float8_e4m3fn), torch.tensor([sa]), torch.tensor([sb])


def fp8_single_operands(case, kind):
    """one fp8 problem behind padded leading dimensions: (A [R, lda], B [R, ldb]) with NaN bytes (0x7f: NaN in e5m2 and in e4m3)
    from columns P / Q on, one 16-byte chunk wider than the rounded-up width; the fp64 product with the scales; the scales"""
    (Pn, Q), R = case.shapes[0], case.R
    a, b, sa, sb = fp8_values(kind, R, Pn, Q, 31 * Pn + Q + R)
    A = torch.full((R, _ru(Pn, 16) + 16), 0x7f, dtype=torch.uint8)
    B = torch.full((R, _ru(Q, 16) + 16), 0x7f, dtype=torch.uint8)
    A[:, :Pn], B[:, :Q] = a.view(torch.uint8), b.view(torch.uint8)
    A, B = A.view(torch.float8_e5m2), B.view(torch.float8_e4m3fn)
    assert bool(torch.isnan(A[:, Pn:].float()).all()) and bool(torch.isnan(B[:, Q:].float()).all())
    return A, B, (a.double().T @ b.double()) * (sa.double().item() * sb.double().item()), sa, sb


def group_operands(case, kind):
    """per problem (A, B, fp64 product, sum |a||b|, scale_a, scale_b): columns of one [R, *] draw per operand, so that every problem has its own
    values and every operand a leading dimension far wider than its matrix, with other problems' (finite) values behind it.
    fp8 "exact": A integers in [-4, 4] (exact in e5m2), B in [-8, 8] (exact in e4m3), scales 0.5 and 4; "randn": 3 N and N
    rounded to e5m2 / e4m3 with the scales of tests/test_gpu_fp8.py."""
    al = 16
    wa = sum(_ru(Pn, al) for Pn, _ in case.shapes)
    wb = sum(_ru(Q, al) for _, Q in case.shapes)
    g = torch.Generator().manual_seed(len(case.shapes) * 1000 + case.R + (7 if kind == "exact" else 0))
    if kind == "exact":
        A = torch.randint(-4, 5, (case.R, wa), generator=g).float()
        B = torch.randint(-8 if case.f8 else -4, (8 if case.f8 else 4) + 1, (case.R, wb), generator=g).float()
    else:
        A = torch.randn(case.R, wa, generator=g) * (3.0 if case.f8 else 1.0)
        B = torch.randn(case.R, wb, generator=g)
    A = A.to(torch.float8_e5m2 if case.f8 else torch.bfloat16)
    B = B.to(torch.float8_e4m3fn if case.f8 else torch.bfloat16)
    out, oa, ob = [], 0, 0
    for i, (Pn, Q) in enumerate(case.shapes):
        a, b = A[:, oa:oa + Pn], B[:, ob:ob + Q]
        sa, sb = ((0.5, 4.0) if kind == "exact" else (0.37 + 0.01 * (i % 20), 1.9 - 0.02 * (i % 20))) if case.f8 else (1.0, 1.0)
        sa, sb = torch.tensor([sa]), torch.tensor([sb])                # (fp32: the factor the kernel multiplies with)
        s = sa.double().item() * sb.double().item()
        ad, bd = a.double(), b.double()
        out.append((a, b, (ad.T @ bd) * s, (ad.abs().T @ bd.abs()) * s, sa, sb))
        oa, ob = oa + _ru(Pn, al), ob + _ru(Q, al)
    return A, B, out
