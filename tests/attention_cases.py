"""The attention launch plan of csrc/attention.hip (attn_plan) as the tests read it, the block orders of csrc/attention_mfma.hip
restated in Python, the case table of tests/test_gpu_attention_instances.py, the case grid of the plan's golden file and the
chunked fp64 reference the GPU cases share -- TEST INFRASTRUCTURE (CPU).

The six attention entries launch what attn_plan returns, and the library reports that plan through the diagnostic entry
dg_debug_attn_plan: pure host code that never launches, so the calls below carry made-up addresses (aligned or misaligned on
purpose, never dereferenced) and nothing here needs a GPU.  ``supported``, ``order``, ``grid`` and ``instances`` read it.
Five inputs pick what a launch of the bf16 MFMA attention runs: the block order (0 plain when nblk % 4 != 0, 1 equal-cost pairs,
2 heavy first), which of two conditions chose order 2 (16 blocks or more -- "length" -- or more workgroups than 3 x #CUs x 1.1
-- "size"), inside order 1 the slot rotation k = (blockIdx / #CUs) % 3, whether tiles, keep bits, the fp8 copy and the document
starts are present, and dg_xcd_remap with a grid that is no multiple of 8.  ``item`` restates the DEVICE function ``attn_item``
(with ``dg_xcd_remap``) and ``rotations`` the values of k it reaches; tests/test_attention_cases_host.py shows the port to be a
bijection onto the (batch * head, block) pairs for every order and that ``CASES(ncu)`` reaches every (order, reason, rotation)
and every (order, instance) pair; the GPU tests then assert, with the CU count of the device they run on, that each case is
the case it is named for.

tests/golden/attn_plan.json holds, for every call of GRID in order, what the commit BEFORE attn_plan existed did for the same
arguments: its return code, per launch the kernel instance with grid, block, dynamic LDS and the host-set kernel parameters, and
what its four queries answered.  It was recorded from that commit's own entries with the launches of its attention units replaced
by a recorder (the kernel expression as spelled at the launch site, normalised to the spelling of the row names), not from
the code under test; "grid_sha" ties it to GRID, which therefore changes only together with a new recording from that commit.

Instance names: the kernel's name with every template argument of its row written out, no spaces (the non-DOC rows leave the
DOC argument out)."""
import collections
import ctypes as C
import functools
import hashlib
import struct

import numpy as np
import torch

from oracle import parity as P
from oracle import rng_ref

TILE, HD = 32, 64
FORMS = ("tiles", "recompute", "keep_bits")
FP8 = (None, "both", "only8")
SEED, STEP, SITE = 77, 3, 4
F32, BF16 = 0, 1
NCUS = (64, 104, 256, 304)


# ---------------------------------------------------------------------------------------------------------------------
# a call of the library and the library's own plan of it
# ---------------------------------------------------------------------------------------------------------------------
# made-up addresses, 256-byte aligned and distinct
ADDR = dict(qkv=0x1000000, out=0x2000000, dout=0x3000000, lse=0x4000000, dqkv=0x5000000, workspace=0x6000000, rng_state=0x7000000,
            keep_bits=0x8000000, starts=0x9000000, q8=0xA000000, hist3=0xB000000, step_state=0xC000000, scale_inv=0xD000000)
FP8_FIELDS = ("q8", "hist3", "step_state", "scale_inv")


class Call(collections.namedtuple("Call", "bwd B T NH H dtype p ncu rng keep ws fp8 starts null odd")):
    """one call of dg_attn_fwd_doc / dg_attn_bwd_doc (the other four entries pass NULL for fp8 or starts) planned for ``ncu``
    compute units.  rng: rng_state present; keep: None, or keep bits of "exact" size (dg_attn_keep_bits_bytes), one byte "short";
    ws (backward): "full" (dg_attn_bwd_workspace_bytes), "delta" (B * NH * T floats), one byte short of either ("full-1",
    "delta-1"); fp8: None, "both", "only8"; null: operands (fp8.<field> for a field of the struct) passed as NULL; odd: operands
    8 bytes off their alignment."""
    __slots__ = ()

    @property
    def name(self):
        parts = ["bwd" if self.bwd else "fwd", f"{self.B}x{self.T}x{self.NH}x{self.H}", f"dt{self.dtype}", f"p{self.p:g}", f"cu{self.ncu}"]
        parts += [k for k in ("rng", "starts") if getattr(self, k)] + [f"{k}={getattr(self, k)}" for k in ("keep", "ws", "fp8") if getattr(self, k)]
        return "/".join(parts + [f"null={n}" for n in self.null] + [f"odd={n}" for n in self.odd])


def call(bwd, B, T, NH, H=HD, dtype=BF16, p=0.0, ncu=256, rng=None, keep=None, ws="full", fp8=None, starts=False, null=(), odd=()):
    return Call(bool(bwd), B, T, NH, H, dtype, float(p), ncu, p > 0 if rng is None else rng, keep, ws if bwd else None, fp8, starts,
                tuple(null), tuple(odd))


@functools.lru_cache(maxsize=1)
def _lib():
    from drakegpt_amd import _lib as L
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    L.lib.dg_debug_attn_plan.argtypes = [i, vp, vp, vp, vp, vp, vp, i64, i, i, i, i, C.c_float, vp, i, vp, i64, C.POINTER(L.AttnFp8Out), vp, i,
                                         C.POINTER(i64), C.POINTER(C.c_char_p)]
    L.lib.dg_debug_attn_plan.restype = i
    return L


def arguments(c, lib=None):
    """dict of the arguments of the entry: the addresses (None: NULL), the byte counts and the fp8 struct (or None).  ``lib``: the
    library whose queries size the keep bits and the workspace (default: the package's)"""
    L = _lib()
    lib = lib or L.lib
    a = {k: (None if k in c.null else v + (8 if k in c.odd else 0)) for k, v in ADDR.items()}
    shape = (c.B, c.T, c.NH, c.H, c.dtype)
    if not c.rng:
        a["rng_state"] = None
    if not c.starts:
        a["starts"] = None
    assert c.keep in (None, "exact", "short"), c.keep
    a["keep_bits_bytes"] = 0
    if c.keep is None:
        a["keep_bits"] = None
    else:
        a["keep_bits_bytes"] = int(lib.dg_attn_keep_bits_bytes(*shape)) - (c.keep == "short")
    a["workspace_bytes"] = 0
    if c.bwd:
        n = {"full": int(lib.dg_attn_bwd_workspace_bytes(*shape)), "delta": c.B * c.NH * c.T * 4}[c.ws.split("-")[0]]
        a["workspace_bytes"] = n - c.ws.endswith("-1")
    a["fp8"] = None
    if c.fp8:
        f = [None if "fp8." + k in c.null else a[k] + (8 if "fp8." + k in c.odd else 0) for k in FP8_FIELDS]
        a["fp8"] = L.AttnFp8Out(*f, int(c.fp8 == "only8"))
    return a


Launch = collections.namedtuple("Launch", "name grid block lds nblk n_items balance rot_div drop thr inv_keep keep tile_off rng_is_qkv site sinv starts")
Plan = collections.namedtuple("Plan", "rc family mfma_ok fp8_out_ok keep_bytes workspace_bytes nblk n_items balance reason rot_div grid block "
                                      "n_launch drop thr inv_keep keep tiles tile_off dq_no_drop passes keys launches")
REASONS = (None, "length", "size")
ONE = struct.unpack("<I", struct.pack("<f", 1.0))[0]


@functools.lru_cache(maxsize=None)
def plan(c):
    """the library's plan of a Call.  launches: what each launch of the call is given, in the terms of the golden file -- the dQ
    launch of a call without dropout runs with threshold 0, scale 1, site 0 and its key read from qkv, the dK/dV launch never
    gets the fp8 copy's scale_inv."""
    L = _lib()
    a = arguments(c)
    out, names = (C.c_int64 * 32)(), (C.c_char_p * 2)()
    L.check(L.lib.dg_debug_attn_plan(int(c.bwd), a["qkv"], a["out"], a["dout"], a["lse"], a["dqkv"], a["workspace"], a["workspace_bytes"],
                                     c.B, c.T, c.NH, c.H, c.p, a["rng_state"], c.dtype, a["keep_bits"], a["keep_bits_bytes"],
                                     C.byref(a["fp8"]) if a["fp8"] is not None else None, a["starts"], c.ncu, out, names), "dg_debug_attn_plan")
    v = list(out)
    n = v[13]
    launches = []
    for i in range(n):
        ps, key, lds, sinv = v[21 + 4 * i:25 + 4 * i]
        sub = ps == 1 and v[20]
        launches.append(Launch(names[i].decode(), v[11], v[12], lds, *v[6:9], v[10], v[14], 0 if sub else v[15], ONE if sub else v[16], v[17], v[19],
                               int(bool(sub)), 0 if sub else SITE, sinv, int(c.starts)))
    return Plan(*v[:21], tuple(v[21 + 4 * i] for i in range(n)), tuple(v[22 + 4 * i] for i in range(n)), tuple(launches))


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, read from the plan; attn_item restated
# ---------------------------------------------------------------------------------------------------------------------
def blocks(T):
    return (T + TILE - 1) // TILE


def supported(B, T, NH, H=HD):
    """dg_attn_mfma_supported: the shape fits the MFMA kernels"""
    return bool(plan(call(0, B, T, NH, H)).mfma_ok)


def size_limit(ncu):
    """a launch of more workgroups than this is "more than one residency": the bound the CU-dependent shapes of CASES are built around"""
    return 3 * ncu * 11 // 10


def grid(B, T, NH):
    return plan(call(0, B, T, NH)).grid


def order(B, T, NH, ncu):
    """(balance, why): (0, None), (1, None), (2, "length") or (2, "size").  Both conditions may hold: "length" is the one that
    holds at any size, so it is named first."""
    p = plan(call(0, B, T, NH, ncu=ncu))
    assert p.rc == 0 and p.family == 1, p
    return p.balance, REASONS[p.reason]


def rotations(B, T, NH, ncu):
    """the values of k = (blockIdx.x / rot_div) % 3 an order 1 launch reaches (empty for the other orders)"""
    p = plan(call(0, B, T, NH, ncu=ncu))
    if p.balance != 1:
        return frozenset()
    return frozenset((b // p.rot_div) % 3 for b in range(0, p.grid, p.rot_div))


def xcd_remap(orig, nwg):
    """dg_xcd_remap (common.h)"""
    nx = 8
    q, r, xcd = nwg // nx, nwg % nx, orig % nx
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + orig // nx


def item(order, blockIdx, wave, B, NH, nblk, ncu, grid):
    """attn_item: (bh, blk, valid) of wave ``wave`` of workgroup ``blockIdx``.  The forward and dQ kernels take blk as their
    query block in orders 1 and 2 and nblk - 1 - blk in order 0; the dK/dV kernels take the mirror image as their key block."""
    if order == 0:
        it = blockIdx * 4 + wave
        return it // nblk, it % nblk, it < B * NH * nblk
    wpq = nblk >> 2
    if order == 2:
        n_bh = B * NH
        cls = blockIdx // n_bh
        return blockIdx % n_bh, nblk - 1 - (4 * cls + wave), cls < wpq
    wg = xcd_remap(blockIdx, grid)
    g, bh = wg % wpq, wg // wpq
    k = (blockIdx // ncu) % 3
    slot = wave if k == 0 else ((0x3201 >> (4 * wave)) & 3) if k == 1 else (wave + 1) & 3
    j = g + wpq if slot >> 1 else g
    return bh, (j if slot & 1 else nblk - 1 - j), bh < B * NH


def instances(B, T, NH, p, ncu, form, fp8=None, doc=False):
    """(forward, dQ, dK/dV) instance names of one forward + backward of the given backward form.
    form "tiles": P | dS tiles from the dQ pass, dropout hashed again; "recompute" (tile_scratch=False): no tiles, the dK/dV pass
    recomputes the scores; "keep_bits": tiles, and the forward (keep=True) leaves its keep decisions for the dQ pass.
    fp8 "both" / "only8": the fp8 entry points (the same instances: only8 is a run-time flag); their forward needs the keep
    bits whenever it drops, whether or not the backward is given them, and their backward needs the tiles.  As drakegpt_amd.ops
    calls the entries: keep bits are allocated with dropout only, the forward never writes only8."""
    assert form in FORMS and fp8 in FP8 and supported(B, T, NH)
    kb = "exact" if p > 0 and (form == "keep_bits" or fp8) else None
    f = plan(call(0, B, T, NH, p=p, ncu=ncu, keep=kb, fp8="both" if fp8 else None, starts=doc))
    kb = "exact" if p > 0 and form == "keep_bits" else None
    b = plan(call(1, B, T, NH, p=p, ncu=ncu, keep=kb, ws="delta" if form == "recompute" else "full", fp8=fp8, starts=doc))
    if f.rc or b.rc:
        raise ValueError(f"rejected: forward {f.rc}, backward {b.rc}")
    return f.launches[0].name, b.launches[0].name, b.launches[1].name


def runs(p, fp8):
    """the (form, fp8) combinations the GPU tests launch for a case at dropout p"""
    r = [(f, None) for f in FORMS]
    if fp8:
        r += [("keep_bits", "both"), ("keep_bits", "only8")] if p > 0 else [("tiles", "both"), ("tiles", "only8")]
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "name B T NH ps fp8 order reason rotations note")):
    """ps: the dropout probabilities the case runs at; fp8: also through the fp8 entry points; order / reason / rotations:
    what the case is named for, asserted against ``order`` and ``rotations`` with the CU count of the device"""
    __slots__ = ()

    @property
    def draw(self):
        return DRAW.get(self.name, 0)

    @property
    def n_items(self):
        return self.B * self.NH * blocks(self.T)

    @property
    def invalid_waves(self):
        return 4 * grid(self.B, self.T, self.NH) - self.n_items


def rotation_batch(ncu):
    """B of the rotation case (T = 250, NH = 3: grid = 6 B): the grid in (2 ncu, size_limit], half way into the third dispatch
    round, and no multiple of 8"""
    B = -(-5 * ncu // 12)
    while B % 4 == 0:
        B += 1
    return B


def size_shape_4(ncu):
    """(B, NH) of the heavy-first-by-size case at four blocks: B * NH > size_limit, B * NH % 8 != 0"""
    NH = 23
    B = size_limit(ncu) // NH + 1
    while B * NH % 8 == 0:
        B += 1
    return B, NH


def size_shape_8(ncu):
    """(B, NH) of the heavy-first-by-size case at eight blocks: the smallest B * NH with 2 B NH > size_limit"""
    n = size_limit(ncu) // 2 + 1
    NH = next(h for h in (4, 3, 2, 1) if n % h == 0)
    return n // NH, NH


ALL3 = frozenset((0, 1, 2))
NONE = frozenset()


def CASES(ncu):
    Br = rotation_batch(ncu)
    B4, NH4 = size_shape_4(ncu)
    B8, NH8 = size_shape_8(ncu)
    return [
        Case("one-tile-2", 1, 2, 1, (0.0, 0.2), False, 0, None, NONE, "one tile, two rows of it; three invalid waves"),
        Case("one-tile-32", 2, 32, 3, (0.0, 0.2), False, 0, None, NONE, "one full tile; 6 items: two invalid waves"),
        Case("plain-ragged", 3, 66, 3, (0.2,), False, 0, None, NONE, "27 items, 3 blocks, 2-row last tile, one invalid wave"),
        Case("plain-5-blocks", 2, 160, 2, (0.0, 0.2), True, 0, None, NONE, "order 0, all forms, fp8"),
        Case("pairs-small", 2, 128, 3, (0.0,), True, 1, None, frozenset((0,)), "order 1 without dropout, fp8 without keep bits"),
        Case("rotation", Br, 250, 3, (0.2,), True, 1, None, ALL3, "order 1, rotations 0, 1 and 2; remap with an uneven grid"),
        Case("heavy-size-4", B4, 126, NH4, (0.2,), True, 2, "size", NONE, "order 2 by size, one class"),
        Case("heavy-size-8", B8, 256, NH8, (0.0,), False, 2, "size", NONE, "order 2 by size, two classes"),
        Case("heavy-length", 1, 512, 3, (0.0, 0.2), True, 2, "length", NONE, "order 2 by length, 16 blocks"),
        Case("heavy-length-ragged", 1, 482, 3, (0.0, 0.2), False, 2, "length", NONE, "16 blocks, 2-row last tile"),
    ]


NAMES = [c.name for c in CASES(256)]
CASE_P = [(c.name, p) for c in CASES(256) for p in c.ps]


def case(name, ncu):
    return next(c for c in CASES(ncu) if c.name == name)


# ---------------------------------------------------------------------------------------------------------------------
# the calls of the plan's golden file: the smallest arguments that reach each branch of attn_plan
# ---------------------------------------------------------------------------------------------------------------------
MFMA_SHAPE = (2, 128, 3, HD)       # order 1 at every CU count of NCUS
GENERIC_SHAPE = (2, 40, 3, 32)


def _grid():
    out, seen = [], set()

    def add(*a, **k):
        c = call(*a, **k)
        if c not in seen:
            seen.add(c)
            out.append(c)

    def both(*a, **k):
        add(0, *a, **k)
        add(1, *a, **k)

    # the ten shapes of CASES at every CU count.  At 256: both dropout settings x plain / document mask x every form of either
    # pass; elsewhere the forms whose instance depends on the block order, with dropout
    for ncu in NCUS:
        for cs in CASES(ncu):
            s = (cs.B, cs.T, cs.NH)
            for p in ((0.0, 0.2) if ncu == 256 else (0.2,)):
                for st in (False, True):
                    for kb in ((None, "exact") if ncu == 256 else ("exact",)):
                        add(0, *s, p=p, ncu=ncu, keep=kb, starts=st)
                        add(1, *s, p=p, ncu=ncu, keep=kb, starts=st)
                        add(1, *s, p=p, ncu=ncu, keep=kb, ws="delta", starts=st)
                        if ncu == 256:
                            add(0, *s, p=p, ncu=ncu, keep="exact", fp8="both", starts=st)
                            add(1, *s, p=p, ncu=ncu, keep=kb, fp8="both", starts=st)
    # the boundaries of the MFMA family
    for s in ((1, 2, 1, HD), (1, 255, 1, HD), (1, 256, 1, 128), (0, 2, 1, HD), (1, 65534, 1, HD), (1, 65536, 1, HD), (2, 46342, 1, HD),
              (1, 2, 0, HD), (1, 0, 1, HD), (-1, 2, 1, HD)):
        both(*s)
    # the generic family: head sizes, dtypes (7: none), the limits on T and H, the 32-bit element index
    for dt in (BF16, F32, 7):
        for T in (40, 4096, 4097):
            both(1, T, 2, 32, dt)
        for H in (64, 300, 256, 257, 0):
            both(1, 40, 2, H, dt)
        both(2, 40, 3, 32, dt, p=0.2, starts=True)
        both(2, 40, 3, 32, dt, starts=True, ws="delta")
        both(2, 40, 3, 32, dt, p=0.2, rng=False)
    both(4, 4096, 64, 32, F32)
    both(4, 4096, 63, 32, F32)
    for s in (MFMA_SHAPE, GENERIC_SHAPE):
        # dropout: with and without rng_state, out of range
        for p in (0.0, 0.2):
            for rng in (False, True):
                both(*s, p=p, rng=rng)
                add(1, *s, p=p, rng=rng, ws="delta")
        for p in (1.0, -0.1):
            both(*s, p=p, rng=True)
        # keep bits: absent, exact, one byte short, misaligned; without dropout
        for kb, odd in ((None, ()), ("exact", ()), ("short", ()), ("exact", ("keep_bits",))):
            both(*s, p=0.2, keep=kb, odd=odd)
            both(*s, p=0.0, keep=kb, odd=odd)
            add(1, *s, p=0.2, keep=kb, odd=odd, ws="delta")
        # workspace: full, delta only, one byte short of each, misaligned, null
        for ws in ("full", "delta", "full-1", "delta-1"):
            add(1, *s, ws=ws)
            add(1, *s, ws=ws, odd=("workspace",))
        add(1, *s, null=("workspace",))
        # the fp8 copy: present, only8, each field null in turn, misaligned, with dropout but no keep bits, without tiles
        for fp8 in ("both", "only8"):
            both(*s, fp8=fp8)
            both(*s, fp8=fp8, p=0.2, keep="exact")
            both(*s, fp8=fp8, p=0.2)
            add(1, *s, fp8=fp8, ws="delta")
            add(1, *s, fp8=fp8, ws="full-1")
        for f in FP8_FIELDS:
            both(*s, fp8="both", null=("fp8." + f,))
            both(*s, fp8="both", odd=("fp8." + f,))
        add(1, *s, fp8="both", p=0.2, keep="exact", odd=("keep_bits",), null=("fp8.q8",))        # the backward names the keep bits first
        add(1, *s, fp8="both", p=0.2, keep="exact", odd=("keep_bits",), ws="delta")
        # the document mask: with the delta-only workspace, with a misaligned keep pointer
        both(*s, starts=True, ws="delta")
        both(*s, starts=True, ws="delta", p=0.2, keep="exact", odd=("keep_bits",))
        both(*s, starts=True, fp8="both", p=0.2)
        # every required pointer null or misaligned in turn
        for k in ("qkv", "out", "lse", "dout", "dqkv"):
            both(*s, null=(k,))
            both(*s, odd=(k,))
        both(*s, p=1.0, rng=True, odd=("keep_bits",), keep="exact")
    return out


GRID = _grid()
GRID_SHA = hashlib.sha256("\n".join(c.name for c in GRID).encode()).hexdigest()[:16]


# ---------------------------------------------------------------------------------------------------------------------
# operands and the reference, once per (case, p), computed in chunks over the batch
# ---------------------------------------------------------------------------------------------------------------------
CHUNK_ELEMS = 1 << 22          # (batch, head, query, key) elements per chunk: 32 MB per fp64 score tensor


def keep_slab(p, start, stop):
    """rng_ref.keep_mask for the linear indices [start, stop) (start even) of the site the cases use"""
    assert start % 2 == 0
    idx = np.arange(start, stop, dtype=np.uint64)
    r = rng_ref.element_hash(rng_ref.site_key(SEED, STEP, SITE), idx >> np.uint64(1))
    field = np.where((idx & np.uint64(1)) == 1, r >> np.uint64(16), r & np.uint64(0xFFFF))
    return (field >= np.uint64(rng_ref.threshold(p))).astype(np.float32)


# The operand draw of a case (default 0).  "heavy-length-ragged": draw 0 has a group -- head 2, query row 1 -- whose dq nearly
# cancels (norm 0.09 against a median of 0.8) and whose expected error from the one rounding that dominates there (delta read
# from the bf16 output, see dq_conditioning) is 9.5e-2 of it, where the rounding model happened to draw 1.1e-2 and, with three
# heads to take a maximum over, set a bound of 4.9e-2; the kernels drew 6.2e-2 (measured, all three forms alike).  The
# criterion that rejects such operands reads the reference alone: tests/test_attention_cases_host.py.
DRAW = {"heavy-length-ragged": 1}


def operands(B, T, NH, draw=0):
    """(qkv [B*T, 3*NH*64], dout [B*T, NH*64]) ~ N(0, 1), bf16"""
    g = torch.Generator().manual_seed(T * 7 + HD + 1000 * B + NH + 10007 * draw)
    C = NH * HD
    return torch.randn(B * T, 3 * C, generator=g).bfloat16(), torch.randn(B * T, C, generator=g).bfloat16()


def delta_noise(R, k, dout, n, T, NH):
    """rms of the error a group of dq [n, NH, T] inherits from delta = rowsum(dout * out) being taken from the bf16-ROUNDED
    output, as the kernels and the rounding model take it: d dq / d delta = -(P k) * scale, delta's error is the sum of the
    output's rounding errors (uniform within half an ulp <= 2^-9 |out|, rms 2^-9 |out| / sqrt 3; none where out is a bf16
    number already: query row 0 without dropout) times dout.  From the fp64 reference alone."""
    do = P.f64(dout).view(n, T, NH, HD).permute(0, 2, 1, 3)
    out = R["Pd"] @ R["v"]
    inexact = (P.rb(out) != out).double()
    sd = (do * out * inexact).square().sum(-1).sqrt() * 2.0 ** -9 / 3 ** 0.5
    return (R["P"] @ k).norm(dim=-1) * HD ** -0.5 * sd


def dq_conditioning(ref, B, T, NH):
    """largest ratio over the groups of dq of 3 x the rms error the group inherits from delta's rounding (relative, with
    rowwise_rel's denominators) to the group's bound.  Above 1 the bound, a maximum over the rounding model's draws at
    B * NH x 33 groups, says less than the distribution those draws come from: the operands are ill-conditioned for the test."""
    den = ref["dq"].reshape(-1, HD).norm(dim=1)
    den = den.clamp_min(max(0.1 * den.median().item(), ref["floors"]["dq"], 1e-300))
    sig = ref["delta_noise"].permute(0, 2, 1).reshape(-1) / den
    return (3 * sig / ref["bounds"]["dq"].clamp_min(1e-300)).max().item()


@functools.lru_cache(maxsize=2)
def reference(B, T, NH, p, draw=0):
    """dict(qkv, dout; fp64: out, lse, dq, dk, dv, env (attention_fwd_envelope), dead [B, NH, T] (rows whose kept
    probabilities are all dropped; None at p = 0), delta_noise [B, NH, T], floors (denominator floors of the gradients' groups: 0 but for T = 2), bounds
    (attention_bwd_bounds_by_position against the bf16 rounding model), model_worst (the model's worst group per gradient)).  Nothing returned is modified by the tests."""
    qkv, dout = operands(B, T, NH, draw)
    C = NH * HD
    nb = max(1, CHUNK_ELEMS // (NH * T * T))
    tril = torch.tril(torch.ones(T, T, dtype=torch.float64))
    parts = collections.defaultdict(list)
    for b0 in range(0, B, nb):
        b1 = min(B, b0 + nb)
        n = b1 - b0
        keep = None
        if p > 0:
            keep = torch.from_numpy(keep_slab(p, b0 * NH * T * T, b1 * NH * T * T).reshape(n, NH, T, T)).double()
            parts["dead"].append((keep * tril).sum(-1) == 0)
        q, d = qkv[b0 * T:b1 * T], dout[b0 * T:b1 * T]
        R = P.attention_fp64(q, d, n, T, NH, HD, keep, p)
        M = P.attention_fp64(q, d, n, T, NH, HD, keep, p, model=True)
        parts["env"].append(P.attention_fwd_envelope(R))
        parts["lse"].append(R["lse"])
        parts["delta_noise"].append(delta_noise(R, P._split(q, n, T, NH, HD)[1], d, n, T, NH))
        for k in ("out", "dq", "dk", "dv", "dq_mag", "dk_mag", "dv_mag"):
            parts[k].append(R[k])
        for k in ("dq", "dk", "dv"):
            parts["m" + k].append(M[k])
    ref = {k: torch.cat(v, 0) for k, v in parts.items()}
    model = {k: ref.pop("m" + k) for k in ("dq", "dk", "dv")}
    ref.setdefault("dead", None)
    # rowwise_rel judges a group against 0.1 x the median group norm.  Where that median is exactly zero (T = 2: two groups of
    # dq, the first one zero in fp64) it is no scale, and the bound would be the model's rounding noise over 1e-300: there the
    # denominators are floored as for structured operands (parity.structured_floor).
    ref["floors"] = {k: P.structured_floor(ref, k, HD) if ref[k].reshape(-1, HD).norm(dim=1).median().item() == 0 else 0.0
                     for k in ("dq", "dk", "dv")}
    ref["bounds"] = P.attention_bwd_bounds_by_position(ref, model, B, T, NH, HD, floors=ref["floors"])
    ref["model_worst"] = {k: P.rowwise_rel(model[k], ref[k], HD, ref["floors"][k]).max().item() for k in ("dq", "dk", "dv")}
    for k in ("dq_mag", "dk_mag", "dv_mag"):
        del ref[k]
    ref.update(qkv=qkv, dout=dout)
    assert ref["out"].shape == (B * T, C) and ref["lse"].shape == (B, NH, T)
    return ref


def slab(x, B, T, NH, b, h, thirds):
    """the (b, h) slab of a packed [B*T, thirds*NH*64] tensor as the packed tensor of a (1, T, 1) launch: [T, thirds*64]"""
    return x.view(B, T, thirds, NH, HD)[b, :, :, h].reshape(T, thirds * HD).contiguous()
