"""drakegpt_amd/csrc/elementwise.hip, branch by branch: every scalar fallback, ragged edge, tail loop and workgroup cap of the
embedding, cast, transpose, dropout-backward and reduction kernels against torch on the CPU -- bit-exact where the operation is
exact, fp64 with a derived bound otherwise.  A case's id (or docstring) quotes the condition in the kernel source that it exists
to reach, so a change to a dispatch shows which cases have to move.

Every output is a view inside a larger buffer filled with a sentinel (``Guarded``); after the launch everything outside the
view must still hold the sentinel bit for bit, which is the out-of-bounds check of this file.

Bounds (u = 2^-24, one fp32 rounding), none of them taken from a kernel's output:
  * a sum of k fp32 terms in any order: k * u * sum |term| (embedding gradients, reduce_sum);
  * dropout-backward: fp32 output one rounding of dy * 1 / (1 - p), asserted as 2^-23 |ref|; bf16 output one bf16 rounding
    (oracle/parity.py); column sums of M such terms: (M + 1) * u * sum |ref|, per partial row (rows + 1) * u * sum |ref|;
  * row softmax: the suite's 1e-6 (tests/test_gpu_ops.py), here per row; row sums within V * 2^-23 of 1.

Measured on MI355X with DG_TEST_REPORT=1 (largest error / bound over the cases of a group; exact comparisons have no entry):

  embedding backward   dtok (k u sum |dx|): fp32 dx 0.48, bf16 dx 0.011;  dpos (B u sum |dx|): fp32 dx 0.64, bf16 dx 0.28
                       clamped ids: dtok 0.46, dpos 0.43;  single-output calls: dtok 0.36, dpos 0.46
  dropout bwd, fp32 in g fp32 0.50 (the one rounding), g bf16 1.00 (0.996: a bf16 store alone reaches its bound),
                       partial rows 0.47, column sums 0.028
  dropout bwd, bf16 in g bf16 0.97, partial rows 0.022, column sums 0.0083
  softmax rows         0.18 of 1e-6 per row;  row sums 0.014 of V 2^-23
  reduce_sum           7.8e-5 of n u sum |x| (the integer-valued input is exact)
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16
DG_ERR_ARG = -1

PAD = 64                                   # sentinel elements on either side of an output; a multiple of 8: 16-byte alignment is kept
_INT = {F32: torch.int32, BF16: torch.int16}
_SENTINEL = {F32: 0x7FC0DEAD, BF16: 0x5A5A}            # a NaN with a payload; a fixed pattern (1.5e16) no kernel here produces
_NAME = {F32: "f32", BF16: "bf16"}


def _ops():
    from drakegpt_amd import ops
    return ops


def _lib():
    from drakegpt_amd import _lib
    return _lib


def _report(name, use):
    if os.environ.get("DG_TEST_REPORT"):
        print(f"[elementwise] {name}: error / bound {use:.3g}", flush=True)


class Guarded:
    """``t``: an output view carved out of a sentinel-filled buffer, ``skew`` elements past an aligned start.  check(): every
    element the view does not cover (the bands in front and behind, the padding between the rows of a strided view) still
    holds the sentinel.  Bits are compared, NaN != NaN."""

    def __init__(self, dev, dtype, numel, carve=lambda b: b, skew=0):
        lo, n = PAD + skew, PAD + skew + numel + PAD
        self.bits = torch.full((n,), _SENTINEL[dtype], dtype=_INT[dtype], device=dev)
        self.covered = torch.zeros(n, dtype=torch.bool, device=dev)
        self.t = carve(self.bits.view(dtype)[lo:lo + numel])
        carve(self.covered[lo:lo + numel]).fill_(True)

    def check(self, name):
        bad = (self.bits != _SENTINEL[self.t.dtype]) & ~self.covered
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements written outside the view, first at buffer offset {int(bad.nonzero()[0])} (view starts at {PAD})"

    def untouched(self, name):
        bad = self.bits != _SENTINEL[self.t.dtype]
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} elements written, none expected"


def assert_bits(got, ref, name):
    """got (device) == ref (CPU) bit for bit; where ref is NaN, any NaN but the sentinel, which is what an element that was
    never written holds"""
    g, r = got.detach().cpu().contiguous(), ref.contiguous()
    assert g.dtype == r.dtype and g.shape == r.shape, (name, g.dtype, r.dtype, g.shape, r.shape)
    gi = g.view(_INT[g.dtype])
    bad = torch.where(torch.isnan(r), ~torch.isnan(g) | (gi == _SENTINEL[g.dtype]), gi != r.view(_INT[r.dtype]))
    if bool(bad.any()):
        at = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ, first at {at}: got {g[at].item()!r}, expected {r[at].item()!r}")


def assert_within(got, ref, bound, name):
    """|got - ref| <= bound for every element (fp64, bound >= 0 of ref's shape; a zero bound asks for equality).  Returns the
    largest error / bound."""
    g, r, b = got.detach().double().cpu(), ref.double(), bound.double()
    assert g.shape == r.shape == b.shape, (name, g.shape, r.shape, b.shape)
    err = (g - r).abs()
    bad = ~(err <= b)                                   # a NaN left in the output offends
    if bool(bad.any()):
        flat = torch.where(bad, torch.nan_to_num(err - b, nan=float("inf")), torch.zeros_like(err)).reshape(-1).argmax()
        at = tuple(int(i) for i in torch.unravel_index(flat, r.shape)) if r.dim() else ()
        raise AssertionError(f"{name}: {int(bad.sum())} of {r.numel()} elements outside their bound; worst at {at}: got {g[at].item():.9g}, "
                             f"ref {r[at].item():.9g}, allowed {b[at].item():.3g}")
    use = torch.where(b > 0, err / b, torch.zeros_like(err)).max().item() if r.numel() else 0.0
    _report(name, use)
    return use


def _ptr(t):
    return None if t is None else t.data_ptr()


def _padded(dev, x, ld, skew=0):
    """x [R, N] on the device as a view of a [R, ld] buffer that starts ``skew`` elements into its allocation; what lies between
    the rows is NaN, so a kernel that reads past a row's N columns into a sum is seen"""
    R, N = x.shape
    buf = torch.full((skew + R * ld,), float("nan"), dtype=x.dtype, device=dev)
    v = buf[skew:].view(R, ld)[:, :N]
    v.copy_(x)
    return v


# ----------------------------------------------------------------------------------------------
# 1. embedding forward: bit-exact against tok[idx] + pos[:T]
# ----------------------------------------------------------------------------------------------
EMBED_FWD = [   # B, T, C, V, with_pos, elements by which x misses 16-byte alignment
    pytest.param(3, 5, 7, 11, True, 0, id="C=7: C%4!=0 -> embed_fwd_kernel<1>"),
    pytest.param(3, 5, 30, 11, True, 0, id="C=30: C%4!=0 -> embed_fwd_kernel<1>, lanes 30..63 idle"),
    # 200 % 4 == 0: with aligned pointers this width takes the vector kernel in one lane round; x one float off does what the case is for
    pytest.param(3, 5, 200, 11, True, 1, id="C=200, !dg_aligned16(x) -> embed_fwd_kernel<1>, cv=200 > 3*64 -> four lane rounds"),
    pytest.param(3, 5, 202, 11, True, 0, id="C=202: C%4!=0 -> embed_fwd_kernel<1>, cv=202 > 3*64 -> four lane rounds"),
    pytest.param(3, 5, 260, 11, True, 0, id="C=260: embed_fwd_kernel<4>, cv=65 -> two lane rounds, the last with one lane"),
    pytest.param(5, 3281, 256, 80, True, 0, id="B*T=16405, C=256: grid > 4096 capped, 16384 waves < M -> a second row per wave"),
    pytest.param(3, 5, 7, 11, False, 0, id="pos=None, embed_fwd_kernel<1>"),
    pytest.param(3, 5, 260, 11, False, 0, id="pos=None, embed_fwd_kernel<4>"),
]


@pytest.mark.parametrize("B,T,C,V,with_pos,skew", EMBED_FWD)
def test_embed_fwd(dev, B, T, C, V, with_pos, skew):
    ops = _ops()
    g = torch.Generator().manual_seed(C)
    idx = torch.randint(0, V, (B, T), generator=g)
    tok = torch.randn(V, C, generator=g)
    pos = torch.randn(T + 3, C, generator=g) if with_pos else None
    out = Guarded(dev, F32, B * T * C, lambda b: b.view(B, T, C), skew=skew)
    assert out.t.data_ptr() % 16 == 4 * skew
    ops.embed_fwd(idx.to(dev), tok.to(dev), pos.to(dev) if with_pos else None, out=out.t)
    assert_bits(out.t, tok[idx] + pos[:T] if with_pos else tok[idx], "x")
    out.check("x")


@pytest.mark.parametrize("C", [pytest.param(7, id="embed_fwd_kernel<1>"), pytest.param(12, id="embed_fwd_kernel<4>")])
def test_embed_clamps_ids_outside_the_table(dev, C):
    """`v = v < 0 ? 0 : (v >= V ? V - 1 : v)` in embed_fwd_kernel and embed_bwd_tok_kernel: the kernels' documented answer to
    a bad id ("never fault on bad input").  By direct call: ops.check_ids refuses such ids on the module path.  No other id
    selects row 0 or row V - 1, so those rows hold the clamped ids' contributions alone."""
    ops, L = _ops(), _lib()
    B, T, V = 2, 4, 6
    g = torch.Generator().manual_seed(C)
    idx = torch.randint(1, V - 1, (B, T), generator=g)
    idx[0, 1], idx[1, 2] = -3, V + 5
    clamped = idx.clamp(0, V - 1)
    tok, pos, dx = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g), torch.randn(B, T, C, generator=g)
    idx_d, tok_d, pos_d, dx_d = idx.to(dev), tok.to(dev), pos.to(dev), dx.to(dev)
    out = Guarded(dev, F32, B * T * C, lambda b: b.view(B, T, C))
    assert L.lib.dg_embed_fwd(_ptr(idx_d), _ptr(tok_d), _ptr(pos_d), _ptr(out.t), B, T, C, V, None, 0, ops._stream()) == 0
    assert_bits(out.t, tok[clamped] + pos, "x")
    out.check("x")
    dtok, dpos = Guarded(dev, F32, V * C, lambda b: b.view(V, C)), Guarded(dev, F32, T * C, lambda b: b.view(T, C))
    assert L.lib.dg_embed_bwd(_ptr(idx_d), _ptr(dx_d), L.DG_F32, _ptr(dtok.t), _ptr(dpos.t), B, T, C, V, ops._stream()) == 0
    assert_bits(dtok.t[0], dx[0, 1], "dtok row 0")
    assert_bits(dtok.t[V - 1], dx[1, 2], "dtok row V - 1")
    _check_embed_bwd(dtok, dpos, clamped, dx, "clamped ids")


@pytest.mark.parametrize("C,V,ld", [pytest.param(64, 80, 88, id="C/4*8=128 > ld: `j*8 < ld_onehot` turns lanes 11..15 away"),
                                    pytest.param(44, 80, 88, id="C/4*8 == ld_onehot: the last lane writes the last chunk")])
def test_embed_fwd_onehot(dev, C, V, ld):
    """the one-hot rows of the non-gather entry: exact, columns [V, ld) zero"""
    ops = _ops()
    B, T = 3, 5
    g = torch.Generator().manual_seed(C)
    idx = torch.randint(0, V, (B, T), generator=g)
    idx[0, 0], idx[0, 1] = 0, V - 1
    tok, pos = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    out = Guarded(dev, F32, B * T * C, lambda b: b.view(B, T, C))
    oh = Guarded(dev, BF16, B * T * ld, lambda b: b.view(B * T, ld))
    ops.embed_fwd(idx.to(dev), tok.to(dev), pos.to(dev), out=out.t, onehot=oh.t)
    assert_bits(out.t, tok[idx] + pos, "x")
    ref = torch.zeros(B * T, ld, dtype=BF16)
    ref[torch.arange(B * T), idx.reshape(-1)] = 1.0
    assert_bits(oh.t, ref, "onehot")
    out.check("x"), oh.check("onehot")


@pytest.mark.parametrize("C,V,ld", [pytest.param(64, 80, 84, id="ld_onehot%8!=0"), pytest.param(64, 80, 72, id="ld_onehot<V"),
                                    pytest.param(40, 80, 88, id="C/4*8<ld_onehot (2C<ld)")])
def test_embed_fwd_onehot_rejected_before_launch(dev, C, V, ld):
    ops, L = _ops(), _lib()
    B, T = 3, 5
    idx = torch.zeros((B, T), dtype=torch.int64, device=dev)
    tok, pos = torch.zeros(V, C, device=dev), torch.zeros(T, C, device=dev)
    out, oh = Guarded(dev, F32, B * T * C), Guarded(dev, BF16, B * T * ld)
    assert L.lib.dg_embed_fwd(_ptr(idx), _ptr(tok), _ptr(pos), _ptr(out.t), B, T, C, V, _ptr(oh.t), ld, ops._stream()) == DG_ERR_ARG
    out.untouched("x"), oh.untouched("onehot")


# ----------------------------------------------------------------------------------------------
# 2. embedding backward
# ----------------------------------------------------------------------------------------------
def _check_embed_bwd(dtok, dpos, idx, dx, name):
    """dtok[v, c]: the sum, in any order (fp32 atomics), of the k rows of dx whose id is v: k * u * sum |dx|; a row that no id
    selects has bound 0, i.e. must be the exact zero that zero_f32_kernel wrote.  dpos[t, c]: a fixed-order sum over B."""
    B, T = idx.shape
    C = dx.shape[-1]
    d, ids = dx.double().reshape(B * T, C), idx.reshape(-1)
    if dtok is not None:
        V = dtok.t.shape[0]
        ref = torch.zeros(V, C, dtype=torch.float64).index_add_(0, ids, d)
        mag = torch.zeros(V, C, dtype=torch.float64).index_add_(0, ids, d.abs())
        k = torch.bincount(ids, minlength=V).double().unsqueeze(1)
        assert_within(dtok.t, ref, k * U * mag, name + " dtok")
        dtok.check(name + " dtok")
    if dpos is not None:
        assert_within(dpos.t, d.view(B, T, C).sum(0), B * U * d.view(B, T, C).abs().sum(0), name + " dpos")
        dpos.check(name + " dpos")


EMBED_BWD = [   # B, T, C, V, every id equal
    pytest.param(1, 3, 7, 5, False, id="(1,3,7): T*C%4!=0 -> non-vector pos kernel, B<4: groups g>=B add nothing; V*C%4!=0 -> zero_f32 tail"),
    pytest.param(3, 5, 7, 5, False, id="(3,5,7): non-vector pos kernel, B<4"),
    pytest.param(6, 5, 9, 5, False, id="(6,5,9): non-vector pos kernel, B%4!=0: groups 0,1 sum two rows, 2,3 one"),
    pytest.param(5, 33, 8, 5, False, id="(5,33,8): T*C%4==0 -> vector pos kernel, T*C=264: the second workgroup covers 8 of 256"),
    pytest.param(4, 512, 64, 7, True, id="(4,512,64) every id equal: 2048 atomic adds per element of one row"),
    pytest.param(3, 700, 1000, 50, False, id="(3,700,1000): M*C > 8192*256 -> tok kernel grid capped, grid-stride loop"),
]


@pytest.mark.parametrize("dx_dtype", [F32, BF16], ids=["dx=f32", "dx=bf16"])
@pytest.mark.parametrize("B,T,C,V,equal", EMBED_BWD)
def test_embed_bwd(dev, B, T, C, V, equal, dx_dtype):
    """ids are drawn from [0, V - 1): row V - 1 -- with V*C%4!=0 it holds zero_f32_kernel's scalar tail -- is selected by none
    and must come back as exact zeros out of a buffer that held NaN"""
    ops = _ops()
    g = torch.Generator().manual_seed(B * T + C)
    idx = torch.full((B, T), 3) if equal else torch.randint(0, V - 1, (B, T), generator=g)
    dx = torch.randn(B, T, C, generator=g).to(dx_dtype)
    idx_d, dx_d = idx.to(dev), dx.to(dev)
    dtok, dpos = Guarded(dev, F32, V * C, lambda b: b.view(V, C)), Guarded(dev, F32, T * C, lambda b: b.view(T, C))
    ops.embed_bwd(idx_d, dx_d, dtok.t, dpos.t)
    _check_embed_bwd(dtok, dpos, idx, dx, f"({B},{T},{C}) dx {_NAME[dx_dtype]}")
    again = Guarded(dev, F32, T * C, lambda b: b.view(T, C))
    ops.embed_bwd(idx_d, dx_d, None, again.t, V=V)
    assert torch.equal(again.t.view(torch.int32), dpos.t.view(torch.int32)), "dpos: two calls differ (the order is fixed)"


@pytest.mark.parametrize("which", ["dtok=None", "dpos=None"])
def test_embed_bwd_single_output(dev, which):
    """the output that is not asked for keeps its sentinel"""
    ops = _ops()
    B, T, C, V = 3, 5, 7, 5
    g = torch.Generator().manual_seed(2)
    idx, dx = torch.randint(0, V - 1, (B, T), generator=g), torch.randn(B, T, C, generator=g)
    dtok, dpos = Guarded(dev, F32, V * C, lambda b: b.view(V, C)), Guarded(dev, F32, T * C, lambda b: b.view(T, C))
    if which == "dtok=None":
        ops.embed_bwd(idx.to(dev), dx.to(dev), None, dpos.t, V=V)
        _check_embed_bwd(None, dpos, idx, dx, which)
        dtok.untouched("dtok")
    else:
        ops.embed_bwd(idx.to(dev), dx.to(dev), dtok.t, None)
        _check_embed_bwd(dtok, None, idx, dx, which)
        dpos.untouched("dpos")


# ----------------------------------------------------------------------------------------------
# 3. casts: bit-exact against torch's CPU conversions
# ----------------------------------------------------------------------------------------------
# fp32 patterns on which round-to-nearest-even to bf16 is decided.  fp32 subnormals are left out: the project states nothing
# about them (flush or keep), and this test does not invent a contract.
CAST_TABLE = torch.from_numpy(np.array([
    0x3F808000, 0x3F818000,      # exact ties: down to the even 0x3F80, up to the even 0x3F82
    0x3F808001, 0x3F807FFF,      # one bit above / below the first tie
    0x3F818001, 0x3F817FFF,      # ... the second
    0xBF808000, 0xBF818000,      # the ties, negative
    0x7F7FFFFF, 0xFF7FFFFF,      # FLT_MAX: rounds to +-inf
    0x7F800000, 0xFF800000,      # +-inf
    0x00000000, 0x80000000,      # +-0
    0x7FC00000,                  # a quiet NaN
], dtype=np.uint32).view(np.int32)).view(F32)
CAST_GRID_STRIDE = 4096 * 256 * 4          # n / 4 > 4096 * 256 work items: the grid-stride loop takes a second trip


def _cast_inputs(n):
    """fp32 inputs of length n that carry CAST_TABLE.  Below 4 elements everything is the scalar tail (`i >= n / 4 * 4`): one
    input per chunk of the table, so every entry goes through the tail loop.  From the table's length on: randn with the table
    at the start, at a vector-aligned place in the body and over the last elements, tail included."""
    L = CAST_TABLE.numel()
    if n < 4:
        return [CAST_TABLE.roll(-s)[:n].clone() for s in range(0, L, n)]
    if n < L:
        return [CAST_TABLE.roll(-s)[:n].clone() for s in (0, L - n)]
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    for at in (0, (n // 2) & ~3, n - L):
        x[at:at + L] = CAST_TABLE
    return [x]


@pytest.mark.parametrize("src,dst", [(F32, BF16), (BF16, F32), (F32, F32)], ids=["f32->bf16", "bf16->f32", "f32->f32"])
@pytest.mark.parametrize("n", [pytest.param(1, id="n=1: n<4, tail only"), pytest.param(3, id="n=3: n<4, tail only"),
                               pytest.param(4, id="n=4: one vector item, no tail"), pytest.param(5, id="n=5: n%4=1"),
                               pytest.param(1029, id="n=1029: n%4=1, two workgroups"),
                               pytest.param(CAST_GRID_STRIDE + 1029, id="n=4096*256*4+1029: grid-stride loop + tail")])
def test_cast(dev, n, src, dst):
    ops = _ops()
    for k, x in enumerate(_cast_inputs(n)):
        x = x.to(src)
        out = Guarded(dev, dst, n)
        ops.cast(x.to(dev), dst, out=out.t)
        assert_bits(out.t, x.to(dst), f"cast input {k}")
        out.check(f"cast input {k}")


# ----------------------------------------------------------------------------------------------
# 4. single transpose: out[c, r] = in[r, c], columns [R, ldo) zero
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["to f32", "to bf16"])
@pytest.mark.parametrize("R,Cc,ldi,ldo", [
    pytest.param(130, 70, 77, None, id="[130,70] of [130,77]: ldi>Cc, 3x2 tiles ragged in r and c"),
    pytest.param(64, 64, 64, 72, id="R=Cc=64, ldo=72: r0=64 tile row reads nothing, writes zeros"),
    pytest.param(1, 1, 1, None, id="R=Cc=1"),
])
def test_transpose_cast(dev, R, Cc, ldi, ldo, dtype):
    ops = _ops()
    W = torch.randn(R, Cc, generator=torch.Generator().manual_seed(R))
    if ldo is None:
        gr = 8 if dtype == BF16 else 4
        ldo = (R + gr - 1) // gr * gr
    out = Guarded(dev, dtype, Cc * ldo, lambda b: b.view(Cc, ldo))
    ops.transpose_cast(_padded(dev, W, ldi), dtype, ldo=ldo, out=out.t)
    ref = torch.zeros(Cc, ldo, dtype=dtype)
    ref[:, :R] = W.T.to(dtype)
    assert_bits(out.t, ref, "W^T")
    out.check("W^T")


# ----------------------------------------------------------------------------------------------
# 5. batched bf16 -> bf16 transpose: descriptors that fail `vec` by the pointer test alone, beside aligned ones in one grid
# ----------------------------------------------------------------------------------------------
def test_transpose_bf16_batched_unaligned_base(dev):
    """`vec = (ldi | ldo) % 8 == 0 && (in | out) % 16 == 0`: every ld is a multiple of 8; descriptors 1 and 3 start 1 element
    (2 bytes) and 4 elements (8 bytes) into their buffers on both sides, descriptors 0 and 2 are 16-byte aligned"""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    pairs, refs = [], []
    for R, Cc, ldi, skew in [(200, 72, 72, 0), (130, 72, 72, 1), (64, 64, 64, 0), (50, 40, 48, 4)]:
        W = torch.randn(R, Cc, generator=g).to(BF16)
        ldo = (R + 7) // 8 * 8
        Wt = Guarded(dev, BF16, Cc * ldo, lambda b, Cc=Cc, ldo=ldo: b.view(Cc, ldo), skew=skew)
        W_d = _padded(dev, W, ldi, skew)
        assert W_d.data_ptr() % 16 == 2 * skew and Wt.t.data_ptr() % 16 == 2 * skew
        pairs.append((W_d, Wt.t))
        refs.append((W, Wt, R))
    ops.transpose_cast_batched(*ops.make_transpose_table(pairs, dev), BF16, in_dtype=BF16)
    for k, (W, Wt, R) in enumerate(refs):
        ref = torch.zeros(tuple(Wt.t.shape), dtype=BF16)
        ref[:, :R] = W.T
        assert_bits(Wt.t, ref, f"descriptor {k}")
        Wt.check(f"descriptor {k}")


# ----------------------------------------------------------------------------------------------
# 6. dropout backward + cast (+ column-sum partials), by direct call: ops.dropout_bwd_cast allocates g itself with ldg = N
# ----------------------------------------------------------------------------------------------
SEED, STEP, SITE = 5, 3, 2


def _keep(p, M, N):
    from oracle import rng_ref
    return torch.from_numpy(rng_ref.keep_mask(SEED, STEP, SITE, p, M * N).reshape(M, N)).double()      # element index m * N + c


def _dropbwd(dev, dy, N, p, out_dtype, ldg, G, mask=None):
    """one dg_dropout_bwd_cast launch.  ldg = 0: no g (want_g=False); G = 0: no partials.  Partial rows are N + 3 apart."""
    ops, L = _ops(), _lib()
    M, ps = dy.shape[0], N + 3
    g = Guarded(dev, out_dtype, M * ldg, lambda b: b.view(M, ldg)[:, :N]) if ldg else None
    part = Guarded(dev, F32, G * ps, lambda b: b.view(G, ps)[:, :N]) if G else None
    rng = ops.new_rng_state(SEED, dev, STEP)
    rc = L.lib.dg_dropout_bwd_cast(_ptr(dy), ops.dt_code(dy.dtype), dy.stride(0), _ptr(g.t) if g else None, ldg, ops.dt_code(out_dtype), M, N, float(p),
                                   _ptr(rng) if p > 0 else None, SITE, _ptr(mask), mask.stride(0) if mask is not None else 0,
                                   _ptr(part.t) if part else None, ps if part else 0, G, ops._stream())
    assert rc == 0, rc
    return g, part


def _check_dropbwd(dev, g, part, ref, G, name):
    """ref: fp64 dy * keep / (1 - p) (* relu mask), exact zeros where an element is dropped or masked"""
    from oracle import parity as P
    ops = _ops()
    M, N = ref.shape
    if g is not None:
        got = g.t.cpu()
        assert bool((got[ref == 0] == 0).all()), f"{name}: a dropped element is not exactly zero"
        if got.dtype == F32:
            assert_within(got, ref, 2.0 ** -23 * ref.abs(), name + " g")
        else:
            _report(name + " g", P.assert_within_rounding(got, ref, P.single_rounding_envelope(ref, 1), 1, name + " g"))
        g.check(name + " g")
    if part is not None:
        rp = (M + G - 1) // G                           # rows_per_partial(); partial rows past ceil(M / rp) sum nothing: zeros
        rows = torch.zeros(G * rp, N, dtype=torch.float64)
        rows[:M] = ref
        assert_within(part.t, rows.view(G, rp, N).sum(1), (rp + 1) * U * rows.abs().view(G, rp, N).sum(1), name + " partials")
        cs = Guarded(dev, F32, N)
        ops.reduce_partials(part.t, N + 3, G, cs.t, N)
        assert_within(cs.t, ref.sum(0), (M + 1) * U * ref.abs().sum(0), name + " column sums")
        part.check(name + " partials"), cs.check(name + " column sums")


DROP_F32 = [   # M, N, lddy, ldg (0: want_g=False), G (0: no partials), ld of the relu mask (0: none)
    pytest.param(37, 7, 8, 7, 3, 0, id="(37,7) lddy=8: c=4 has c+3>=N -> full==false; c=0 full && vec_in; ldg%4!=0 -> !vec_out"),
    pytest.param(64, 258, 259, 260, 3, 0, id="(64,258) lddy=259: full && !vec_in (lddy%4!=0), vec_out; blockIdx.y=1 ragged"),
    pytest.param(64, 258, 259, 261, 3, 0, id="(64,258) lddy=259, ldg=261: !vec_in, !vec_out, ldg>N"),
    pytest.param(1000, 384, 385, 384, 31, 0, id="(1000,384) lddy=385: full && !vec_in, rows_per=33"),
    pytest.param(64, 258, 259, 260, 3, 263, id="(64,258) relu_mask a strided view, ldmask=263"),
    pytest.param(64, 258, 259, 0, 3, 0, id="(64,258) want_g=False: g==nullptr, column sums only"),
    pytest.param(1000, 40, 41, 40, 0, 0, id="M=1000 no partials: default n_partials = 1 below M=1024"),
    pytest.param(1100, 40, 41, 40, 0, 0, id="M=1100 no partials: default n_partials = M/64 = 17, rows_per=65"),
    pytest.param(70000, 4, 5, 4, 0, 0, id="M=70000 no partials: default n_partials = M/64 = 1093 capped at 1024, rows_per=69"),
    pytest.param(37, 7, 8, 7, 50, 0, id="(37,7) n_partials=50 > M: rows_per=1, partial rows 37..49 written as zeros"),
]


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["g=f32", "g=bf16"])
@pytest.mark.parametrize("p", [0.0, 0.2], ids=["p=0", "p=0.2"])
@pytest.mark.parametrize("M,N,lddy,ldg,G,ldmask", DROP_F32)
def test_dropout_bwd_cast_f32_in(dev, M, N, lddy, ldg, G, ldmask, p, out_dtype):
    """dropbwd_cast_kernel<float, TO, DROP>"""
    g = torch.Generator().manual_seed(M + N)
    dy = torch.randn(M, N, generator=g)
    mask = torch.randn(M, N, generator=g) if ldmask else None
    ref = dy.double() * _keep(p, M, N) / (1 - p)
    if mask is not None:
        ref = ref * (mask > 0)
    dy_d, mask_d = _padded(dev, dy, lddy), _padded(dev, mask, ldmask) if ldmask else None
    out, part = _dropbwd(dev, dy_d, N, p, out_dtype, ldg, G, mask_d)
    _check_dropbwd(dev, out, part, ref, G, f"f32 in, {_NAME[out_dtype]} out ({M},{N}) p={p}")
    if part is not None:
        _, again = _dropbwd(dev, dy_d, N, p, out_dtype, ldg, G, mask_d)
        assert torch.equal(again.t.view(torch.int32), part.t.view(torch.int32)), "partials: two calls differ (the order is fixed)"


DROP_BF16 = [  # M, N, lddy (= ldg), G with partials
    pytest.param(3, 8, 8, 2, id="vec8 N=8: RL=256, rows_per<RL"),
    pytest.param(100, 8, 8, 2, id="vec8 N=8: RL=256, M=100: rows_per<RL"),
    pytest.param(3, 24, 24, 2, id="vec8 N=24: nc8=3, RL=85, thread 255 has rl>=RL"),
    pytest.param(100, 24, 24, 2, id="vec8 N=24: RL=85, rows_per<4*RL: the four-in-flight loop is not entered"),
    pytest.param(3, 40, 40, 2, id="vec8 N=40: nc8=5, RL=51, thread 255 has rl>=RL"),
    pytest.param(100, 40, 40, 2, id="vec8 N=40: RL=51, rows_per<4*RL"),
    pytest.param(3, 2048, 2048, 2, id="vec8 N=2048: RL=1, rows_per<4*RL"),
    pytest.param(100, 2048, 2048, 2, id="vec8 N=2048: RL=1, four rows in flight + remainder"),
    pytest.param(1000, 384, 392, 31, id="vec8 (1000,384) lddy=392>N: RL=5, rows_per=33"),
    pytest.param(100, 12, 12, 2, id="generic bf16: N%8!=0 (N=12)"),
    pytest.param(37, 2056, 2056, 2, id="generic bf16: N>2048 (N=2056), 9 column blocks, the last ragged"),
    pytest.param(100, 24, 28, 2, id="generic bf16: lddy%8!=0 (lddy=28)"),
]


@pytest.mark.parametrize("partials", [True, False], ids=["partials", "no partials: lds=0"])
@pytest.mark.parametrize("p", [0.0, 0.2], ids=["p=0", "p=0.2"])
@pytest.mark.parametrize("M,N,ld,G", DROP_BF16)
def test_dropout_bwd_cast_bf16_in(dev, M, N, ld, G, p, partials):
    """dropbwd_cast_vec8_kernel (N%8==0 && N<=2048 && lddy%8==0 && ldg%8==0, 16-byte aligned) and its fallback
    dropbwd_cast_kernel<bf16, bf16>"""
    dy = torch.randn(M, N, generator=torch.Generator().manual_seed(M + N)).to(BF16)
    ref = dy.double() * _keep(p, M, N) / (1 - p)
    dy_d = _padded(dev, dy, ld)
    G = G if partials else 0
    out, part = _dropbwd(dev, dy_d, N, p, BF16, ld, G)
    _check_dropbwd(dev, out, part, ref, G, f"bf16 in, bf16 out ({M},{N}) p={p}")
    if p == 0.0:
        assert_bits(out.t, dy, "p=0: g is dy")
    if partials:
        _, again = _dropbwd(dev, dy_d, N, p, BF16, ld, G)
        assert torch.equal(again.t.view(torch.int32), part.t.view(torch.int32)), "partials: two calls differ (the order is fixed)"


@pytest.mark.parametrize("p", [0.0, 0.2], ids=["p=0", "p=0.2"])
def test_dropout_bwd_cast_bf16_fallback_keeps_what_vec8_keeps(dev, p):
    """the same [100, 24] data with lddy = 24 (vec8: one hash word per element pair) and lddy = 28 (lddy%8!=0: the generic
    kernel, one dg_keep per element): the same keep decisions, hence the same bits"""
    M, N = 100, 24
    dy = torch.randn(M, N, generator=torch.Generator().manual_seed(1)).to(BF16)
    a, _ = _dropbwd(dev, _padded(dev, dy, 24), N, p, BF16, 24, 0)
    b, _ = _dropbwd(dev, _padded(dev, dy, 28), N, p, BF16, 24, 0)
    assert torch.equal(a.t.view(torch.int16), b.t.view(torch.int16))
    a.check("vec8"), b.check("generic")


# ----------------------------------------------------------------------------------------------
# 7. row softmax and scalar sum
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V,ld", [pytest.param(1, 1, 1, id="(1,1,1): V<64, one lane"), pytest.param(5, 63, 63, id="(5,63,63): V<64, M%4!=0"),
                                    pytest.param(6, 65, 80, id="(6,65,80): V%64!=0, ldl!=V, M%4!=0"),
                                    pytest.param(3, 50257, 50304, id="(3,50257,50304): V%64!=0, ldl!=V, M<4")])
def test_softmax_rows(dev, M, V, ld):
    """row 0 carries a common offset of +1e4; the last row (M > 1) has every second entry at -inf.  By direct call: ops.softmax_rows
    allocates probs itself."""
    from oracle import parity as P
    ops, L = _ops(), _lib()
    x = torch.randn(M, V, generator=torch.Generator().manual_seed(V))
    x[0] += 1e4
    if M > 1:
        x[M - 1, ::2] = float("-inf")
    probs = Guarded(dev, F32, M * ld, lambda b: b.view(M, ld)[:, :V])
    x_d = _padded(dev, x, ld)
    assert L.lib.dg_softmax_rows(_ptr(x_d), ld, _ptr(probs.t), ld, M, V, ops._stream()) == 0
    got, ref = probs.t.cpu(), x.double().softmax(-1)
    _report(f"softmax ({M},{V},{ld})", P.assert_rowwise(got, ref, V, 1e-6, "softmax_rows") / 1e-6)
    assert_within(got.double().sum(1), torch.ones(M, dtype=torch.float64), torch.full((M,), V * 2.0 ** -23, dtype=torch.float64), "softmax row sums")
    assert bool((got[torch.isinf(x)] == 0).all()), "a -inf logit has a probability other than 0"
    probs.check("probs")


@pytest.mark.parametrize("n", [pytest.param(1, id="n=1"), pytest.param(63, id="n=63: one partly filled wave"),
                               pytest.param(1025, id="n=1025: n%1024=1, thread 0 takes a second element"),
                               pytest.param(100003, id="n=100003: n%1024!=0")])
def test_reduce_sum(dev, n):
    ops = _ops()
    x = torch.randn(n, generator=torch.Generator().manual_seed(n))
    out = Guarded(dev, F32, 1, lambda b: b[0])
    ops.reduce_sum(x.to(dev), 0.5, out=out.t)           # scaling by a power of two is exact
    assert_within(out.t, 0.5 * x.double().sum(), 0.5 * n * U * x.double().abs().sum(), f"reduce_sum n={n}")
    k = torch.randint(-8, 9, (n,), generator=torch.Generator().manual_seed(n)).float()
    ops.reduce_sum(k.to(dev), 0.5, out=out.t)           # every partial sum is an integer below 2^24: exact in any order, so a
    assert_bits(out.t, (0.5 * k.double().sum()).float(), "integer-valued terms")      # term left out shows at every n
    out.check("out")
