"""csrc/attention_mfma.hip: its host dispatch and its block orders restated in Python, the case table of
tests/test_gpu_attention_instances.py and the chunked fp64 reference those cases share -- TEST INFRASTRUCTURE (CPU).

Five inputs pick what a launch of the bf16 MFMA attention runs: the block order ``fill`` chooses (0 plain when nblk % 4 != 0,
1 equal-cost pairs, 2 heavy first), which of two conditions chose order 2 (16 blocks or more -- "length" -- or more workgroups
than 3 x #CUs x 1.1 -- "size"), inside order 1 the slot rotation k = (blockIdx / #CUs) % 3, whether tiles, keep bits and the fp8
copy are present, and dg_xcd_remap with a grid that is no multiple of 8.  ``order`` and ``rotations`` follow ``fill``, ``item``
is ``attn_item`` (with ``dg_xcd_remap``), ``instances`` follows ``dg_attn_fwd_mfma``, ``attn_dq_launch`` and
``dg_attn_bwd_mfma`` line by line.

Nothing in the suite can observe WHICH kernel a launch ran, so no test checks a kernel's name on the device.  Instead
tests/test_attention_cases_host.py holds this restatement to the source: the names ``instances`` can return are the
hipLaunchKernelGGL targets read from the text of the kernel file, the port of ``attn_item`` is a bijection onto the (batch *
head, block) pairs for every order, and ``CASES(ncu)`` reaches every (order, reason, rotation) and every (order, instance)
pair; the GPU tests then assert, with the CU count of the device they run on, that each case is the case it is named for.

Instance names: the kernel's name with every template argument written out (defaults included), no spaces."""
import collections
import functools

import numpy as np
import torch

from oracle import parity as P
from oracle import rng_ref

TILE, HD = 32, 64
FORMS = ("tiles", "recompute", "keep_bits")
FP8 = (None, "both", "only8")
SEED, STEP, SITE = 77, 3, 4


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch
# ---------------------------------------------------------------------------------------------------------------------
def blocks(T):
    return (T + TILE - 1) // TILE


def supported(B, T, NH, H=HD):
    """dg_attn_mfma_supported"""
    return (H == HD and B > 0 and T > 0 and T % 2 == 0 and NH > 0 and B * NH * T * T < 1 << 32 and T < 1 << 24
            and 3 * NH * HD < 1 << 24 and T * 3 * NH * HD < 1 << 32)


def size_limit(ncu):
    """a launch of more workgroups than this is "more than one residency" (C integer arithmetic: 3 * ncu * 11 / 10)"""
    return 3 * ncu * 11 // 10


def grid(B, T, NH):
    return (B * NH * blocks(T) + 3) // 4


def order(B, T, NH, ncu):
    """(p.balance, why): (0, None), (1, None), (2, "length") or (2, "size").  Both conditions may hold: "length" is the one that
    holds at any size, so it is named first."""
    nblk = blocks(T)
    balance = 1 if nblk % 4 == 0 else 0
    if not balance:
        return 0, None
    if nblk >= 16:
        return 2, "length"
    if B * NH * (nblk // 4) > size_limit(ncu):
        return 2, "size"
    return 1, None


def rotations(B, T, NH, ncu):
    """the values of k = (blockIdx.x / rot_div) % 3 an order 1 launch reaches (empty for the other orders)"""
    if order(B, T, NH, ncu)[0] != 1:
        return frozenset()
    return frozenset((b // ncu) % 3 for b in range(0, grid(B, T, NH), ncu))


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


def _b(x):
    return "true" if x else "false"


def instances(B, T, NH, p, ncu, form, fp8=None):
    """(forward, dQ, dK/dV) instance names of one forward + backward of the given backward form.
    form "tiles": P | dS tiles from the dQ pass, dropout hashed again; "recompute" (tile_scratch=False): no tiles, the dK/dV pass
    recomputes the scores; "keep_bits": tiles, and the forward (keep=True) leaves its keep decisions for the dQ pass.
    fp8 "both" / "only8": the fp8 entry points (the same instances: only8 is a run-time flag); their forward needs the keep
    bits whenever it drops, whether or not the backward is given them, and their backward needs the tiles."""
    assert form in FORMS and fp8 in FP8 and supported(B, T, NH)
    o, _ = order(B, T, NH, ncu)
    drop = p > 0
    if fp8 and form == "recompute":
        raise ValueError("rejected: the fp8 copy of dqkv needs the tiles")
    if fp8:
        fwd = f"attn_fwd_mfma_kernel<{_b(drop)},{_b(drop)},true>"
    else:
        fwd = f"attn_fwd_mfma_kernel<{_b(drop)},{_b(drop and form == 'keep_bits')},false>"
    tiles = form != "recompute"
    kb = form == "keep_bits" and drop and tiles            # keep bits are ignored without dropout and without tiles
    # p == 0 launches the same dQ build with threshold 0
    dq = f"attn_bwd_dq_mfma_kernel<{_b(tiles)},{_b(kb)},{_b(bool(fp8))},{_b(tiles and o == 2)}>"
    if tiles and o:
        dkv = "attn_bwd_dkv_tiles_shared_f8_kernel" if fp8 else "attn_bwd_dkv_tiles_shared_kernel"
    elif tiles:
        dkv = "attn_bwd_dkv_tiles_f8_kernel" if fp8 else "attn_bwd_dkv_tiles_kernel"
    else:
        dkv = f"attn_bwd_dkv_mfma_kernel<{_b(drop)}>"
    return fwd, dq, dkv


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
