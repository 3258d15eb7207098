"""csrc/fp8.hip (dg_fp8_amax, dg_fp8_quantize, dg_fp8_quantize_delayed) and the scaling rules of csrc/common.h restated on the
host, and the case tables of tests/test_gpu_fp8_casts.py -- TEST INFRASTRUCTURE (CPU; tests/test_fp8_cases_host.py holds it
against torch's cast, against the library's own plan and against planted defects).

Nothing in the suite can observe WHICH loop a launch took, how many workgroups it had or which of them had work.  The library
therefore reports its own launch plan through a diagnostic entry (dg_debug_fp8_plan: the host function the three entries
themselves call, with the predicate the kernels themselves evaluate; pure host code that runs without a GPU), and the class of
every case below is read from that plan -- there is no second copy of the dispatch here.  The only restatement is ``_partials``,
the device-side map from a unit of work to its workgroup, (i // block) % parts, with the block, the workgroups per segment and the unit size taken
from the plan: tests/test_fp8_cases_host.py holds it against a plain loop, holds the kernel names the plan can return against the
hipLaunchKernelGGL targets read from the source text, and holds the case tables to reach every branch they list.  The GPU tests
then assert, with the addresses of the tensors they pass, that each case is the case it is named for.

Four parts:

  encoder     ``encode``: fp32 -> OCP e4m3fn / e5m2 codes by integer arithmetic on the fp32 bit pattern, round to nearest even
              through the subnormals, the sign of a zero kept, NaN -> the format's NaN.  No torch fp8 dtype is used here.
  arithmetic  ``scale_of`` / ``model_cast`` / ``amax_bits``: what the kernels compute, operation by operation in fp32 -- the amax is
              the integer maximum of the |x| bit patterns (NaN / Inf poison it), scale = min(FMAX / amax, 2^126) (amax 0: 1, NaN /
              Inf: NaN), q = encode(clamp(fp32(x) * scale)) with a comparing clamp (NaN stays NaN, +-Inf saturates),
              scale_inv = fp32(1 / scale).
  geometry    ``quantize_geometry`` / ``delayed_geometry`` / ``amax_geometry``: readers of the plan -- which path a launch takes
              (wide: 16 elements and one 16-byte store per lane and trip; narrow: 8 elements, and why), its grid, the trips of the
              busiest thread and the workgroups without work -- and, with ``_partials``, the partial maximum every workgroup
              records (``delayed_partials`` / ``amax_partials``).
  cases       the smallest sizes that reach each branch, the operand builders (all bf16 patterns, the rounding boundaries of
              either format for fp32 sources, random segments with a planted maximum and 1e6 fillers in the gaps) and the guard
              bands: every source and every output lies between BAND sentinel elements, the output view filled with the sentinel
              too, so a skipped, late or stray store is a byte that differs.

``compare`` is the one function the GPU test judges a launch with; the host test feeds it model outputs with planted defects.
NaN codes are compared as a class (e5m2 has six, e4m3fn two: OCP leaves payload and sign to the implementation); every other
byte is compared exactly.

NOT COVERED, because no sensible size reaches it (named, not approximated):
  * dg_fp8_quantize without segments: the cap of the grid needs tens of millions of elements.
  * dg_fp8_quantize with segments: the cap of blocks_per_seg needs a mean segment of a million elements, the lower clamp to 1
    needs n < n_seg (impossible with segments of at least 8 elements).
  * an ``x`` that is not 16-byte aligned: both entries refuse it (DG_ERR_ARG), so that term of ``wide`` is always true;
    ``q`` 8-byte aligned is the only alignment reason a case can have.
  * segments whose table entries are not multiples of 8: outside the documented contract of the entry."""
import collections
import ctypes as C
import functools

import numpy as np
import torch

E4M3, E5M2 = "e4m3", "e5m2"
FORMATS = (E4M3, E5M2)
F32, BF16 = "f32", "bf16"
DTYPES = (BF16, F32)
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
ESZ = {F32: 4, BF16: 2}
FMAX = {E4M3: 448.0, E5M2: 57344.0}
# exponent bits, mantissa bits, bias, NaN code (sign bit clear)
SPEC = {E4M3: (4, 3, 7, 0x7F), E5M2: (5, 2, 15, 0x7F)}
SCALE_CAP = np.float32(2.0 ** 126)

AMAX_PARTS = 256            # DG_FP8_AMAX_PARTS: the public ABI constant (include/drakegpt_hip.h; tests/test_abi.py holds it)

BAND = 64                   # sentinel elements on either side of every buffer (64 fp32 / bf16 / bytes: 16-byte alignment is kept)
Q_SENTINEL = 0xA5
X_SENTINEL = 1.0e6          # also the filler between segments: it must not leak into any amax
STALE = 123.0               # what the history slot to be written holds before the launch


# ---------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------
def is_nan_code(codes, fmt):
    """e4m3fn: S.1111.111; e5m2: S.11111.{01,10,11}"""
    c = np.asarray(codes, dtype=np.uint8) & 0x7F
    return c == 0x7F if fmt == E4M3 else c > 0x7C


def canonical(codes, fmt):
    """NaN codes as one class (0x7F); every other byte as it is"""
    c = np.asarray(codes, dtype=np.uint8).copy()
    c[is_nan_code(c, fmt)] = 0x7F
    return c


def encode(values_f32, fmt, rounding="rne", fnuz=False):
    """fp32 values, already scaled and clamped to +-FMAX -> uint8 codes.  Integer arithmetic on the bit pattern.  ``rounding``
    ("trunc", "away": ties away from zero) and ``fnuz`` (bias + 1, no negative zero, NaN = 0x80) exist for the planted
    defects of the host test alone."""
    ebits, mbits, bias, nan = SPEC[fmt]
    if fnuz:
        bias += 1
    v = np.ascontiguousarray(values_f32, dtype=np.float32)
    bits = v.view(np.uint32).astype(np.int64)
    sign = (bits >> 31) << 7
    a = bits & 0x7FFFFFFF
    isnan = a > 0x7F800000
    assert np.all(isnan | (a <= np.float32(FMAX[fmt]).view(np.uint32))), "encode: values beyond +-FMAX (clamp first)"
    a = np.where(isnan, 0, a)
    e32 = a >> 23

    def rnd(x, sh):              # x >> sh with the chosen rounding; sh >= 1 (array or scalar)
        if rounding == "trunc":
            return x >> sh
        if rounding == "away":
            return (x + (1 << (sh - 1))) >> sh
        return (x + (1 << (sh - 1)) - 1 + ((x >> sh) & 1)) >> sh

    # normal results: round the 23-bit mantissa to mbits, a carry runs into the exponent field by itself; then rebias
    sh_n = 23 - mbits
    normal = rnd(a, sh_n) - ((127 - bias) << mbits)
    # subnormal results: an integer count of 2^(1 - bias - mbits); mant24 * 2^(e32 - 150) / 2^(1 - bias - mbits)
    mant = np.where(e32 > 0, (a & 0x7FFFFF) | 0x800000, 0)
    sh_s = np.clip(151 - bias - mbits - e32, 1, 40)
    sub = rnd(mant, sh_s)
    code = np.where(e32 >= 128 - bias, normal, sub)
    if fnuz:
        out = np.where(isnan, 0x80, np.where(code == 0, 0, code | sign))
    else:
        out = np.where(isnan, nan | sign, code | sign)
    return out.astype(np.uint8)


def decode(codes, fmt):
    """codes -> float64 (NaN / Inf codes included); the inverse the boundary builder and the host test need"""
    ebits, mbits, bias, _ = SPEC[fmt]
    c = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    s = np.where(c & 0x80, -1.0, 1.0)
    e, m = (c & 0x7F) >> mbits, c & ((1 << mbits) - 1)
    val = np.where(e == 0, m * 2.0 ** (1 - bias - mbits), (1 + m * 2.0 ** -mbits) * 2.0 ** (e - bias).astype(np.float64))
    val = np.where(is_nan_code(c, fmt), np.nan, val)
    if fmt == E5M2:
        val = np.where((c & 0x7F) == 0x7C, np.inf, val)
    return s * val


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic, in fp32
# ---------------------------------------------------------------------------------------------------------------------
def to_f32(x):
    """torch bf16 / fp32 tensor (CPU) -> numpy float32, exactly"""
    return x.detach().float().contiguous().view(-1).numpy()


def abs_bits(x_f32):
    return np.ascontiguousarray(x_f32, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)


def amax_bits(x_f32):
    """dg_amax_nan over a tensor: the unsigned maximum of the |x| bit patterns, as a float32 (+0.0 for an empty or all -0.0 one)"""
    b = abs_bits(x_f32)
    return np.uint32(b.max() if b.size else 0).view(np.float32)


def scale_of(amax, fmax):
    """dg_fp8_scale_of: amax == 0: 1; NaN / Inf: NaN; else min(fmax / amax, 2^126) in fp32"""
    amax = np.float32(amax)
    if amax == 0:
        return np.float32(1.0)
    if not amax < np.float32(np.inf):
        return np.float32(np.nan)
    with np.errstate(over="ignore"):
        return np.minimum(np.float32(fmax) / amax, SCALE_CAP)


def scale_inv_of(scale):
    with np.errstate(divide="ignore"):
        return np.float32(1.0) / np.float32(scale)


def clamp(w, fmax):
    """dg_fp8_clamp: two comparisons, so a NaN stays a NaN and +-Inf saturates"""
    f = np.float32(fmax)
    return np.where(w > f, f, np.where(w < -f, -f, w)).astype(np.float32)


def model_cast(x_f32, amax, fmt, **defect):
    """(codes, scale_inv) of a tensor cast with the scale of ``amax``"""
    sc = scale_of(amax, FMAX[fmt])
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.ascontiguousarray(x_f32, dtype=np.float32) * sc
    return encode(clamp(w, FMAX[fmt]), fmt, **defect), scale_inv_of(sc)


# ---------------------------------------------------------------------------------------------------------------------
# the launch geometry: the library's own plan
# ---------------------------------------------------------------------------------------------------------------------
SegGeo = collections.namedtuple("SegGeo", "first len wide why units trips busy idle")
Geo = collections.namedtuple("Geo", "grid bps segs kernel block wgs")
AmaxGeo = collections.namedtuple("AmaxGeo", "grid segs kernel block wgs")
AmaxSeg = collections.namedtuple("AmaxSeg", "first len vec nv tail trips idle")
KIND = {"amax": 0, "quantize": 1, "delayed": 2}
DT_CODE = {F32: 0, BF16: 1}
WHY = ("first", "len", "q_align", "x_align")          # the bits of fp8_narrow_terms, lowest first
BASE = 1 << 20                                         # a made-up 16-byte aligned address for queries without tensors
DG_ERR_ARG = -1


def _cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=1)
def _lib():
    from drakegpt_amd import _lib as L
    lib = L.lib
    lib.dg_debug_fp8_plan.argtypes = [C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64), C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_char_p)]
    lib.dg_debug_fp8_plan.restype = C.c_int
    lib.dg_debug_fp8_constants.argtypes = [C.POINTER(C.c_float)]
    lib.dg_debug_fp8_constants.restype = None
    lib.dg_debug_fp8_scale.argtypes = [C.c_float, C.c_int]
    lib.dg_debug_fp8_scale.restype = C.c_float
    return L


def plan_rc(entry, dtype, n, seg=None, x_addr=BASE, q_addr=BASE):
    """(return code, launch words, segment rows, kernel name) of dg_debug_fp8_plan: what the entry launches for a tensor at these
    byte addresses, or the entry's refusal"""
    ns = len(seg) if seg is not None else 1
    table = (C.c_int64 * (2 * ns))(*[w for row in seg for w in row]) if seg is not None else None
    launch, rows, name = (C.c_int64 * 6)(), (C.c_int64 * (9 * ns))(), C.c_char_p()
    rc = _lib().lib.dg_debug_fp8_plan(KIND[entry], DT_CODE[dtype], n, table, ns, x_addr, q_addr, launch, rows, ns, C.byref(name))
    return rc, list(launch), [list(rows[9 * i:9 * i + 9]) for i in range(ns)], name.value.decode() if name.value else None


def _plan(entry, dtype, n, seg, x_addr, q_addr):
    rc, launch, rows, name = plan_rc(entry, dtype, n, seg, x_addr, q_addr)
    assert rc == 0, f"the entry refuses this call ({rc})"
    assert launch[5] == len(rows) and launch[4] == launch[3] * launch[1]
    return launch, rows, name


def _cast_geometry(entry, dtype, n, seg, x_addr, q_addr):
    (grid, block, bps, wgs, _, _), rows, name = _plan(entry, dtype, n, seg, x_addr, q_addr)
    segs = []
    for first, length, terms, unit, units, tail, trips, busy, idle in rows:
        why = tuple(w for i, w in enumerate(WHY) if terms >> i & 1)
        assert unit == (8 if why else 16) and tail == 0
        segs.append(SegGeo(first, length, not why, why, units, trips, busy, idle))
    return Geo(grid, bps, tuple(segs), name, block, wgs)


def quantize_geometry(dtype, n, seg=None, x_off=0, q_off=0, x_addr=None, q_addr=None):
    """dg_fp8_quantize: x_off / q_off are the byte offsets of the views from a 16-byte boundary (or the real addresses)"""
    return _cast_geometry("quantize", dtype, n, seg, BASE + x_off if x_addr is None else x_addr, BASE + q_off if q_addr is None else q_addr)


def delayed_geometry(dtype, n, x_off=0, q_off=0, x_addr=None, q_addr=None):
    return _cast_geometry("delayed", dtype, n, None, BASE + x_off if x_addr is None else x_addr, BASE + q_off if q_addr is None else q_addr)


def amax_geometry(dtype, n, seg=None, x_addr=BASE):
    (grid, block, _, wgs, _, _), rows, name = _plan("amax", dtype, n, seg, x_addr, 0)
    return AmaxGeo(grid, tuple(AmaxSeg(first, length, unit, units, tail, trips, idle) for first, length, _, unit, units, tail, trips, _, idle in rows),
                   name, block, wgs)


def constants():
    """(FP8_E4M3_MAX, FP8_E5M2_MAX, the cap of the scale) as the library holds them"""
    out = (C.c_float * 3)()
    _lib().lib.dg_debug_fp8_constants(out)
    return tuple(np.float32(v) for v in out)


def lib_scale_of(amax, fmt):
    """dg_fp8_scale_of itself, compiled for the host"""
    return np.float32(_lib().lib.dg_debug_fp8_scale(float(np.float32(amax)), 3 if fmt == E5M2 else 2))


# ---------------------------------------------------------------------------------------------------------------------
# the device-side work map (the one restatement)
# ---------------------------------------------------------------------------------------------------------------------
def _partials(bits, unit, block, parts):
    """unit i (``unit`` elements) belongs to workgroup (i // block) % parts: the maximum of the |x| bit patterns per workgroup"""
    nu = bits.size // unit
    out = np.zeros(parts, dtype=np.uint32)
    if nu:
        per_unit = bits[:nu * unit].reshape(nu, unit).max(axis=1)
        pad = _cdiv(nu, block * parts) * block * parts
        grid = np.zeros(pad, dtype=np.uint32)
        grid[:nu] = per_unit
        out = grid.reshape(-1, parts, block).max(axis=(0, 2))
    return out


def delayed_partials(x_f32, geo):
    """slot.next of fp8_quantize_delayed_kernel, all AMAX_PARTS entries, as float32"""
    return _partials(abs_bits(x_f32), 16 if geo.segs[0].wide else 8, geo.block, geo.wgs).view(np.float32)


def amax_partials(x_f32, seg_geo, geo):
    """parts[seg * PARTS + b] of fp8_amax_kernel for one segment: the vector loop, then the scalar tail (fewer than a vector's
    elements, so workgroup 0 takes all of it)"""
    b = abs_bits(x_f32[seg_geo.first:seg_geo.first + seg_geo.len])
    out = _partials(b, seg_geo.vec, geo.block, geo.wgs)
    if seg_geo.tail:
        out[0] = max(out[0], b[seg_geo.nv * seg_geo.vec:].max())
    return out.view(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# operand builders (torch CPU tensors; cached ones are never modified)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bf16_patterns(finite=True):
    """the 65280 finite bf16 bit patterns in pattern order (a multiple of 16), or the 256 NaN / Inf ones"""
    p = torch.arange(65536, dtype=torch.int32)
    nonfinite = (p & 0x7F80) == 0x7F80
    p = p[~nonfinite] if finite else p[nonfinite]
    return p.to(torch.int16).view(torch.bfloat16)


def code_points(fmt):
    """every positive finite code point of the format, ascending, as float64 (exact in fp32)"""
    c = np.arange(1, 0x7F, dtype=np.uint8)
    v = decode(c, fmt)
    return np.sort(v[np.isfinite(v)])


@functools.lru_cache(maxsize=None)
def boundary_targets(fmt):
    """float32 values in the SCALED domain where the rounding decides: every code point, the midpoint of every pair of neighbours
    (0 | smallest subnormal and FMAX | the code point that would follow included) with its fp32 predecessor and successor, FMAX's
    own neighbours, all mirrored, and +-0.  Padded with zeros to a multiple of 16."""
    pts = code_points(fmt)
    step_top = pts[-1] - pts[-2]
    ladder = np.concatenate([[0.0], pts, [pts[-1] + step_top]])
    mids = ((ladder[:-1] + ladder[1:]) / 2).astype(np.float32)
    assert np.all(mids.astype(np.float64) * 2 == ladder[:-1] + ladder[1:])            # exact in fp32
    pts32 = pts.astype(np.float32)
    top = pts32[-1:]
    pos = np.concatenate([pts32, mids, np.nextafter(mids, np.float32(0)), np.nextafter(mids, np.float32(np.inf)),
                          np.nextafter(top, np.float32(0)), np.nextafter(top, np.float32(np.inf))])
    vals = np.concatenate([pos, -pos, np.array([0.0, -0.0], dtype=np.float32)]).astype(np.float32)
    pad = -vals.size % 16
    return torch.from_numpy(np.concatenate([vals, np.zeros(pad, dtype=np.float32)]))


def boundary_amaxes(fmt):
    """the amax values the boundary set is cast with: FMAX * 2^-k, k in {0, 7, -3} (power-of-two scales 1, 2^7, 2^-3: the
    kernel's product reconstructs the target exactly) and one that is no power of two times FMAX (the fp32 product decides)"""
    f = FMAX[fmt]
    return [("k0", np.float32(f), 1.0), ("k7", np.float32(f * 2.0 ** -7), 2.0 ** 7), ("k-3", np.float32(f * 8.0), 2.0 ** -3),
            ("odd", np.float32(f * 0.3), None)]


def boundary_sources(fmt, amax, scale_pow2):
    """fp32 sources x with x * scale_of(amax) == the boundary targets (exactly, for a power-of-two scale)"""
    t = boundary_targets(fmt)
    if scale_pow2 is not None:
        x = t / scale_pow2
        assert torch.equal(x * scale_pow2, t)
        return x
    return (t.double() / float(scale_of(amax, FMAX[fmt]))).float()


def tiny_amaxes(fmt):
    """amax values below FMAX / FLT_MAX, where FMAX / amax is +Inf in fp32"""
    edge = np.float32(FMAX[fmt]) / np.finfo(np.float32).max
    return [("1e-37", np.float32(1e-37)), ("denormal", np.float32(1e-40)), ("below_edge", np.nextafter(edge, np.float32(0)))]


def tiny_cases():
    """(name, dtype, fmt, amax as the dtype holds it): fp32 sources at all three, bf16 ones where the rounded amax is still
    below the edge"""
    out = []
    for fmt in FORMATS:
        for name, a in tiny_amaxes(fmt):
            for dtype in DTYPES:
                held = np.float32(torch.tensor(float(a), dtype=torch.float32).to(TORCH[dtype]).float().item())
                with np.errstate(over="ignore"):
                    if held > 0 and np.isinf(np.float32(FMAX[fmt]) / held):
                        out.append((f"{name}-{dtype}-{fmt}", dtype, fmt, held))
    return out


def tiny_source(amax, dtype, n=48):
    """a tensor whose amax is ``amax`` (rounded to the dtype), with exact zeros of both signs, halves and random fractions"""
    a = torch.tensor(float(amax), dtype=torch.float32).to(TORCH[dtype])
    g = torch.Generator().manual_seed(17)
    x = (torch.rand(n, generator=g) * 2 - 1).float() * a.float()
    x = x.to(TORCH[dtype])
    x[0::6] = 0.0
    x[3::12] = -0.0
    x[1], x[2] = a, -a / 2
    return x, np.float32(a.float().item())


# ---------------------------------------------------------------------------------------------------------------------
# buffers between guard bands
# ---------------------------------------------------------------------------------------------------------------------
class Banded:
    """a flat tensor of BAND sentinels | off padding | n elements | BAND sentinels; ``view`` is the middle.  ``off`` (elements)
    moves the view off the 16-byte boundary on purpose."""

    def __init__(self, n, dtype, sentinel, off=0, device="cpu"):
        self.n, self.off = n, off
        self.buf = torch.full((BAND + off + n + BAND,), sentinel, dtype=dtype, device=device)

    @property
    def view(self):
        return self.buf[BAND + self.off:BAND + self.off + self.n]

    def to(self, device):
        o = Banded.__new__(Banded)
        o.n, o.off, o.buf = self.n, self.off, self.buf.to(device)
        return o

    def bytes(self):
        return self.buf.detach().cpu().contiguous().view(torch.uint8).numpy().copy()


def source_buffer(x):
    """x (flat CPU tensor) between bands of X_SENTINEL"""
    b = Banded(x.numel(), x.dtype, X_SENTINEL)
    b.view.copy_(x.reshape(-1))
    return b


def output_buffer(n, q_off=0):
    return Banded(n, torch.uint8, Q_SENTINEL, off=q_off)


def expected_q(codes, q_off=0):
    """the whole output buffer as the launch must leave it"""
    b = output_buffer(len(codes), q_off)
    out = b.bytes()
    out[BAND + q_off:BAND + q_off + len(codes)] = codes
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def ulp_apart(a, b):
    """distance in fp32 ulps of two arrays (NaN with NaN: 0; NaN with a number: a large value)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float32)), np.atleast_1d(np.asarray(b, dtype=np.float32))
    na, nb = np.isnan(a), np.isnan(b)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.abs(ia - ib)
    return np.where(na & nb, 0, np.where(na | nb, 1 << 40, d))


def _same_bits(got, want, what):
    g, w = np.ascontiguousarray(got, dtype=np.float32).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}"


def compare(got, want, fmt, what=""):
    """``got`` / ``want``: dicts of numpy arrays.  Exact but for scale_inv (1 ulp) and the class of NaN codes.
      q          the whole output buffer, guard bands included (uint8)
      x          the whole source buffer as bytes
      scale_inv  one fp32 per segment (entries the launch does not write: absent)
      written    (delayed) the history slot this launch records, AMAX_PARTS fp32, with ``amax`` (its maximum) and ``idle``
                 (the workgroups without work) in ``want``
      read       (delayed) the slot it reads
      parts      (amax) every partial, other segments' and untouched ones included
    Returns whether scale_inv is exact."""
    gq, wq = canonical(got["q"], fmt), canonical(want["q"], fmt)
    assert gq.shape == wq.shape
    bad = np.nonzero(gq != wq)[0]
    assert bad.size == 0, (f"{what}: {bad.size} output bytes differ, first at buffer offset {bad[0]} (view starts at "
                           f"{want.get('q_start', BAND)}): got 0x{int(got['q'][bad[0]]):02X}, want 0x{int(want['q'][bad[0]]):02X}")
    assert np.array_equal(got["x"], want["x"]), f"{what}: the source or its guard bands changed"
    exact = True
    if "scale_inv" in want:
        d = ulp_apart(got["scale_inv"], want["scale_inv"])
        assert np.all(d <= 1), f"{what}: scale_inv {got['scale_inv']!r}, want {want['scale_inv']!r} ({d} ulp)"
        exact = bool(np.all(d == 0))
    if "written" in want:
        rec = np.asarray(got["written"], dtype=np.float32)
        rb, ab = rec.view(np.uint32), np.float32(want["amax"]).view(np.uint32)
        assert rb.max() == ab, f"{what}: recorded maximum {rb.max().view(np.float32)!r}, want {want['amax']!r}"
        assert np.all(rb <= ab), f"{what}: a partial maximum outside [0, amax]"
        assert np.all(rb[-want["idle"]:] == 0) if want["idle"] else True, f"{what}: a workgroup without work did not record 0.0"
        _same_bits(rec, want["written"], f"{what}: written slot")
        _same_bits(got["read"], want["read"], f"{what}: read slot")
    if "parts" in want:
        _same_bits(got["parts"], want["parts"], f"{what}: partial maxima")
    return exact


# ---------------------------------------------------------------------------------------------------------------------
# the case tables
# ---------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name entry dtype fmt n q_off step seg expect")

STEPS = (6, 7, 0xFFFFFFFF)          # parity 0, 1, 1; 0xFFFFFFFF advances to 0

# dg_fp8_quantize without segments: (name, n, q_off, expectation of the geometry)
QUANTIZE_FLAT = [
    ("n8", 8, 0, dict(wide=False, why=("len",), trips=1, grid=1)),
    ("n16", 16, 0, dict(wide=True, why=(), trips=1, grid=1)),
    ("n24", 24, 0, dict(wide=False, why=("len",), trips=1, grid=1)),
    ("wide_second_trip", 16 * 1024 * 2 + 16, 0, dict(wide=True, why=(), trips=2, grid=5)),
    ("narrow_by_q", 16 * 1024 * 2 + 16, 8, dict(wide=False, why=("q_align",), trips=4, grid=5)),
    ("narrow_ragged", 8 * 1024 * 5 + 8, 0, dict(wide=False, why=("len",), trips=4, grid=6)),
]

# dg_fp8_quantize_delayed: (name, n, q_off, expectation)
DELAYED = [
    ("n8", 8, 0, dict(wide=False, why=("len",), trips=1, idle=255)),
    ("n16", 16, 0, dict(wide=True, why=(), trips=1, idle=255)),
    ("wide_second_trip", 2 ** 22 + 2 ** 15 + 16, 0, dict(wide=True, why=(), trips=2, idle=0, second=3)),
    ("narrow_second_trip", 2 ** 21 + 8 * 1027, 0, dict(wide=False, why=("len",), trips=2, idle=0)),
    ("narrow_by_q", 2 ** 16, 8, dict(wide=False, why=("q_align",), trips=1, idle=248)),
]

# the segment table, in this order (and reversed): kind -> (first % 16, length)
SEG_SPEC = [("wide", 0, 1024), ("narrow_first", 8, 1024), ("narrow_len", 0, 1032), ("wide_100x", 0, 102400), ("eight", 0, 8),
            ("wide_after", 0, 2048)]
SEG_AMPS = [0.02, 3.0, 0.5, 1e-4, 100.0, 7.0]          # 1e-4 .. 100, one per segment (by position in SEG_SPEC)

# dg_fp8_amax alone: n, where the maximum is planted.  (A second trip of the vector loop needs more than 65536 vectors: 65536 * 4 + 5
# has it for fp32 and not for bf16, which gets 65536 * 8 + 11 for it.)
AMAX_NS = (3, 1003, 65536 * 4 + 5)
AMAX_WHERE = ("tail", "last_vector", "first")


def seg_layout(reverse=False):
    """[(kind, first, len, amp)], total elements: segments in SEG_SPEC order (or reversed), an 8-element gap wherever the next
    segment's ``first % 16`` asks for one, and a 64-element gap after the large segment"""
    spec = list(zip(SEG_SPEC, SEG_AMPS))
    if reverse:
        spec = spec[::-1]
    pos, out = 0, []
    for (kind, mod, length), amp in spec:
        if pos % 16 != mod:
            pos += 8
        out.append((kind, pos, length, amp))
        pos += length
        if kind == "wide_100x":
            pos += 64
    return out, pos + (-pos % 16)


def seg_source(dtype, reverse=False, seed=5):
    """the flat source of a segment case: random segments with a planted maximum each, 1e6 in every gap; (x, table, amaxes)"""
    layout, n = seg_layout(reverse)
    g = torch.Generator().manual_seed(seed + int(reverse))
    x = torch.full((n,), X_SENTINEL, dtype=torch.float32)
    amaxes = []
    for i, (kind, first, length, amp) in enumerate(layout):
        v = torch.randn(length, generator=g) * amp
        peak = torch.tensor(amp * 6.5, dtype=torch.float32).to(TORCH[dtype]).float()
        v[(length * 5) // 7] = peak if i % 2 else -peak
        x[first:first + length] = v
        amaxes.append(np.float32(peak.item()))
    x = x.to(TORCH[dtype])
    for (kind, first, length, amp), a in zip(layout, amaxes):
        assert amax_bits(to_f32(x[first:first + length])) == a
    return x, [(first, length) for _, first, length, _ in layout], amaxes


def planted_source(dtype, n, seed, amp=1.0, where=None):
    """random values with one planted maximum (at ``where``, default two thirds in); (x, amax)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, generator=g) * amp).to(TORCH[dtype])
    peak = torch.tensor(amp * 6.5, dtype=torch.float32).to(TORCH[dtype])
    x[(2 * n) // 3 if where is None else where] = -peak
    assert amax_bits(to_f32(x)) == np.float32(peak.float().item())
    return x, np.float32(peak.float().item())


def quantize_cases():
    out = []
    for dtype in DTYPES:
        for fmt in FORMATS:
            for name, n, q_off, exp in QUANTIZE_FLAT:
                out.append(Case(f"flat-{name}-{dtype}-{fmt}", "quantize", dtype, fmt, n, q_off, None, None, exp))
            for rev in (False, True):
                out.append(Case(f"seg-{'reversed' if rev else 'forward'}-{dtype}-{fmt}", "quantize", dtype, fmt, seg_layout(rev)[1], 0, None,
                                rev, None))
    return out


def delayed_cases():
    out = []
    for dtype in DTYPES:
        for fmt in FORMATS:
            for name, n, q_off, exp in DELAYED:
                out.append(Case(f"{name}-{dtype}-{fmt}", "delayed", dtype, fmt, n, q_off, STEPS[len(out) % 3], None, exp))
    return out


def amax_where(dtype, n, where):
    """the element that holds the planted maximum"""
    V = 16 // ESZ[dtype]
    if where == "tail":
        return n - 1
    if where == "last_vector":
        return max((n // V) * V - 1, 0)
    return 0


def amax_cases():
    out = []
    for dtype in DTYPES:
        for n in AMAX_NS + ((65536 * 8 + 11,) if dtype == BF16 else ()):
            for where in AMAX_WHERE:
                out.append(Case(f"n{n}-{where}-{dtype}", "amax", dtype, None, n, 0, None, None, where))
    return out


def geometry_of(case):
    if case.entry == "quantize":
        seg = None if case.seg is None else [(f, l) for _, f, l, _ in seg_layout(case.seg)[0]]
        return quantize_geometry(case.dtype, case.n, seg, 0, case.q_off)
    if case.entry == "delayed":
        return delayed_geometry(case.dtype, case.n, 0, case.q_off)
    return amax_geometry(case.dtype, case.n)


def read_slot(amax, seed=1):
    """AMAX_PARTS partials below ``amax`` with one entry equal to it: what the slot that is read is seeded with"""
    g = torch.Generator().manual_seed(seed)
    s = (torch.rand(AMAX_PARTS, generator=g) * 0.9).numpy().astype(np.float32) * np.float32(amax)
    s[17] = np.float32(amax)
    return s


# ---------------------------------------------------------------------------------------------------------------------
# what a launch must leave behind, from the model
# ---------------------------------------------------------------------------------------------------------------------
def expect_quantize(x, fmt, q_off=0, table=None, **defect):
    """dg_fp8_amax + dg_fp8_quantize on the flat CPU tensor ``x``: the ``want`` of ``compare`` (q, x, scale_inv, parts)"""
    dtype = BF16 if x.dtype == torch.bfloat16 else F32
    xf = to_f32(x)
    segs = [(0, x.numel())] if table is None else table
    ageo = amax_geometry(dtype, x.numel(), table)
    view = np.full(x.numel(), Q_SENTINEL, dtype=np.uint8)
    sinv, parts = [], []
    for (first, length), sg in zip(segs, ageo.segs):
        p = amax_partials(xf, sg, ageo)
        codes, si = model_cast(xf[first:first + length], amax_bits(p), fmt, **defect)
        view[first:first + length] = codes
        sinv.append(si)
        parts.append(p)
    return dict(q=expected_q(view, q_off), q_start=BAND + q_off, x=source_buffer(x).bytes(), scale_inv=np.array(sinv, dtype=np.float32),
                parts=np.concatenate(parts))


def expect_delayed(x, fmt, q_off, prev, **defect):
    """dg_fp8_quantize_delayed on ``x`` with the read slot ``prev`` (AMAX_PARTS fp32)"""
    dtype = BF16 if x.dtype == torch.bfloat16 else F32
    xf = to_f32(x)
    geo = delayed_geometry(dtype, x.numel(), 0, q_off)
    codes, si = model_cast(xf, amax_bits(prev), fmt, **defect)
    return dict(q=expected_q(codes, q_off), q_start=BAND + q_off, x=source_buffer(x).bytes(), scale_inv=np.array([si], dtype=np.float32),
                written=delayed_partials(xf, geo), read=np.asarray(prev, dtype=np.float32).copy(), amax=amax_bits(xf), idle=geo.segs[0].idle)
