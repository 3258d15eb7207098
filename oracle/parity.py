"""Localized parity checks -- TEST INFRASTRUCTURE ONLY (CPU, fp64).

A whole-tensor Frobenius ratio ``||a - b|| / ||b||`` moves by ``sqrt(wrong / total)`` when a few elements are wrong: one
zeroed (row, head) of an attention gradient, one wrong row of a 40000-row GEMM output or one wrong 16-byte chunk all vanish
under a tolerance sized for bf16 rounding.  This file holds the two kinds of check that do see them:

  * ``assert_within_rounding`` -- EVERY element within ``ulps * 2^-8 * |ref| + envelope`` of the fp64 reference, where the
    envelope is DERIVED from the arithmetic the kernel performs (the functions ``*_envelope`` below, all evaluated in fp64 on
    the test's own operands) and never measured on a kernel's output;
  * ``rowwise_rel`` / ``assert_rowwise`` -- the relative L2 error of every group of trailing elements (an output row; a
    (row, head) of attention), asserted on the MAXIMUM over groups.  Where no closed-form element bound is attempted (the bf16
    attention backward: P, dS and the rounded O all enter) the bound is ``margin x`` the worst group of a CPU model of the
    kernel's documented rounding points (``attention_bf16_model``), a reference-side number.

Number formats: bf16 keeps 8 significand bits, so round-to-nearest moves a value by at most 2^-9 of the power of two below
it, i.e. at most 2^-8 |x| however x sits in its binade; fp32 accumulation of K products is bounded by K * 2^-24 * sum |a||b|.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

Tensor = torch.Tensor
BF16_RN = 2.0 ** -8        # bound on |bf16(x) - x| / |x| for round-to-nearest (one ulp of the binade's lower end, halved)
TILE = 32                  # rows per MFMA tile of the kernels: failures are reported with their tile coordinates


def f64(x: Tensor) -> Tensor:
    return x.detach().double().cpu()


def rb(x: Tensor) -> Tensor:
    """fp64 -> (fp32 ->) bf16 -> fp64: the value a kernel stores when it writes x as bf16."""
    return x.float().bfloat16().double()


def rel(a: Tensor, b: Tensor) -> float:
    """the whole-tensor ratio the suite has always used (kept here for the planted-defect tests)"""
    a, b = f64(a), f64(b)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# --------------------------------------------------------------------------------------
# row-wise
# --------------------------------------------------------------------------------------
def rowwise_rel(got: Tensor, ref: Tensor, group: int, floor: float = 0.0) -> Tensor:
    """relative L2 error per group of ``group`` trailing elements.  Each denominator is floored at 0.1 x the median group norm
    of ``ref``: a legitimately tiny group (the last keys' dk: one query contributes) is judged against the tensor's scale, not
    against itself.  ``floor``: a further absolute floor under the denominators, for tensors whose median is no scale
    (see structured_floor)."""
    g, r = f64(got).reshape(-1, group), f64(ref).reshape(-1, group)
    assert g.shape == r.shape, (g.shape, r.shape)
    den = r.norm(dim=1)
    floor = max(0.1 * den.median().item(), floor, 1e-300)
    err = (g - r).norm(dim=1) / den.clamp_min(floor)
    return torch.where(torch.isfinite(g).all(dim=1), err, torch.full_like(err, float("inf")))


def describe_group(idx: int, groups_per_row: int, T: Optional[int] = None) -> str:
    row, head = divmod(int(idx), groups_per_row)
    t = row % T if T else row
    s = f"group {idx}: row {row}"
    if T:
        s += f" (batch {row // T}, position {t})"
    return s + f", head {head}, 32-row tile {t // TILE} (row {t % TILE} of it)"


def assert_rowwise(got: Tensor, ref: Tensor, group: int, bound: float, name: str = "", T: Optional[int] = None) -> float:
    """max over groups of rowwise_rel < bound; returns the maximum.  ``T``: rows per sequence, for the tile coordinates."""
    e = rowwise_rel(got, ref, group)
    worst = int(e.argmax())
    m = e[worst].item()
    if not m < bound:
        per_row = f64(ref).shape[-1] // group if f64(ref).dim() > 1 else 1
        raise AssertionError(f"{name}: worst group error {m:.3e} >= {bound:.3e} at {describe_group(worst, max(per_row, 1), T)}; "
                             f"{int((e >= bound).sum())} of {e.numel()} groups over the bound")
    return m


# --------------------------------------------------------------------------------------
# element-wise
# --------------------------------------------------------------------------------------
def assert_within_rounding(got: Tensor, ref: Tensor, envelope, ulps: float = 1.0, name: str = "",
                           where: Optional[Tensor] = None) -> float:
    """|got - ref| <= ulps * 2^-8 * |ref| + envelope for EVERY element (of those selected by ``where``).  Returns the largest
    ratio error / bound (<= 1 on success) so that a caller can report how much of the envelope is used."""
    g, r = f64(got), f64(ref)
    assert g.shape == r.shape, (g.shape, r.shape)
    env = envelope if isinstance(envelope, Tensor) else torch.full_like(r, float(envelope))
    bound = ulps * BF16_RN * r.abs() + f64(env).expand_as(r)
    err = (g - r).abs()
    bad = ~(err <= bound)                                   # NaN / inf in got count as offenders
    if where is not None:
        bad &= where.cpu()
    if bool(bad.any()):
        excess = torch.where(bad, torch.nan_to_num(err - bound, nan=float("inf"), posinf=float("inf")), torch.zeros_like(err))
        flat = int(excess.reshape(-1).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), r.shape)) if r.dim() else ()
        row, col = (idx[-2], idx[-1]) if len(idx) >= 2 else (0, idx[-1] if idx else 0)
        raise AssertionError(f"{name}: {int(bad.sum())} of {r.numel()} elements outside the rounding envelope; worst at {idx} "
                             f"(32 x 32 tile ({row // TILE}, {col // TILE}), 8-element chunk {col // 8} of row {row}): "
                             f"got {g.reshape(-1)[flat].item():.6g}, ref {r.reshape(-1)[flat].item():.6g}, "
                             f"allowed {bound.reshape(-1)[flat].item():.3g}")
    ok = bound > 0 if where is None else (bound > 0) & where.cpu()           # (masked, not gathered: these tensors reach 50 M elements)
    return torch.where(ok, err / bound, torch.zeros_like(err)).max().item() if r.numel() else 0.0


def gemm_envelope(A: Tensor, B: Tensor, K: Optional[int] = None, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
                  scale: float = 1.0, keep_scale: Optional[Tensor] = None) -> Tensor:
    """C = A B^T (+ bias) (+ resid) accumulated in fp32: every partial sum is rounded once (2^-24 relative each, K of them on
    a running sum bounded by sum |a||b|), hence |fp32 result - exact| <= K * 2^-24 * (|A| |B|^T + |bias| + |resid|).
    ``scale``: the dequantisation factor of fp8 operands; ``keep_scale``: keep / (1 - p) of a dropout in front of the residual."""
    A, B = f64(A), f64(B)
    K = A.shape[1] if K is None else K
    e = (A.abs() @ B.abs().T) * abs(scale)
    if bias is not None:
        e = e + f64(bias).abs()
    if keep_scale is not None:
        e = e * f64(keep_scale)
    if resid is not None:
        e = e + f64(resid).abs()
    return e * (K * 2.0 ** -24)


def gemm_nt_epilogue_fp64(acc: Tensor, bias: Optional[Tensor] = None, relu: bool = False, sign_mask: Optional[Tensor] = None,
                          relu_mask: Optional[Tensor] = None, keep: Optional[Tensor] = None, p: float = 0.0,
                          residual: Optional[Tensor] = None) -> dict:
    """The epilogue of dg_gemm_nt as csrc/gemm_nt_ws.h describes it, in fp64 on ``acc`` = A B^T (times the fp8 scales), in the
    kernel's order: + bias, ReLU, the one-bit mask (``sign_mask``: 0 / 1 per element), the tensor-valued mask (kept where
    ``relu_mask`` > 0: 0.0 and -0.0 both drop), dropout (``keep`` 0 / 1 per element, times 1 / (1 - p)), + residual.  Returns
    dict(out: the value stored (before the output's rounding), pre: acc + bias, the value whose sign a ReLU decides, bit: out > 0,
    the emitted sign bit, colsum: column sums of out)."""
    v = f64(acc).clone()
    if bias is not None:
        v = v + f64(bias)
    pre = v
    if relu:
        v = v.clamp_min(0.0)
    if sign_mask is not None:
        v = torch.where(f64(sign_mask) != 0, v, torch.zeros_like(v))
    if relu_mask is not None:
        v = torch.where(f64(relu_mask) > 0, v, torch.zeros_like(v))
    if keep is not None:
        v = v * f64(keep) * (1.0 / (1.0 - p))
    if residual is not None:
        v = v + f64(residual)
    return dict(out=v, pre=pre, bit=v > 0, colsum=v.sum(0))


def split_bf16(x: Tensor) -> Tuple[Tensor, Tensor]:
    """hi = bf16(x), lo = bf16(x - hi) of fp32 values, as fp64 (dg_split_bf16 of csrc/gemm_nt_ws.h)"""
    x = x.detach().cpu().float()
    hi = x.bfloat16().float()
    return hi.double(), (x - hi).bfloat16().double()


def x3_emulation(A: Tensor, B: Tensor) -> Tensor:
    """A B^T of precision "bf16x3" with exact sums: lo_a.hi_b + hi_a.lo_b + hi_a.hi_b in fp64 (the lo.lo term is dropped)"""
    (ah, al), (bh, bl) = split_bf16(A), split_bf16(B)
    return al @ bh.T + ah @ bl.T + ah @ bh.T


X3_SPLIT = 3 * 2.0 ** -16 * (1 + 2.0 ** -8)


def x3_envelope(A: Tensor, B: Tensor, K: Optional[int] = None, bias: Optional[Tensor] = None, resid: Optional[Tensor] = None,
                keep_scale: Optional[Tensor] = None) -> Tensor:
    """|bf16x3 result - exact| <= (3 * 2^-16 * (1 + 2^-8) + 3 K * 2^-24) * |A| |B|^T, derived:

    u = 2^-8 is bf16's unit roundoff: 8 significand bits, so the spacing in [2^e, 2^(e+1)) is 2^(e-7) and round-to-nearest moves x
    by at most 2^(e-8) <= u |x|.  The bound is attained: x = 1 + 2^-8 is a tie, hi = 1, lo = 2^-8 = u |x| / (1 + u) -- so
    |lo| <= 2^-9 |x| does not hold for every x, and the constant below is four times the one that premise would give.
    With d = x - hi (exact in fp32), lo = bf16(d), r = d - lo:  |d| <= u |x|,  |lo| <= u (1 + u) |x|,  |r| <= u |d| <= u^2 |x|, and
    a b - (ha hb + ha lb + la hb) = la lb + ra b + (a - ra) rb, hence per product
        |error| <= (u^2 (1 + u)^2 + u^2 + (1 + u^2) u^2) |a||b| <= 3 u^2 (1 + u) |a||b|.
    The bf16 x bf16 products are exact in fp32; the three MFMAs of a K step add 3 K terms to the fp32 accumulator, each add
    rounded once on a running sum bounded by sum |a||b|: 3 K * 2^-24.  ``bias`` / ``resid`` / ``keep_scale`` (keep / (1 - p) times the
    0 / 1 masks in front of the residual): the epilogue's at most three further fp32 roundings, 3 * 2^-24 of the magnitudes they
    act on, which the same coefficient applied to bias and residual covers (3 u^2 > 3 * 2^-24) once K + 1 stands for K."""
    K = f64(A).shape[1] if K is None else K
    plain = bias is None and resid is None and keep_scale is None
    coef = X3_SPLIT + 3 * (K if plain else K + 1) * 2.0 ** -24
    return gemm_envelope(A, B, 1, bias, resid, keep_scale=keep_scale) * (2.0 ** 24 * coef)


def mask_margin(pre: Tensor, envelope: Tensor, max_share: float = 1e-3) -> Tensor:
    """elements whose fp64 pre-activation lies further from zero than the envelope: the sign (ReLU, sign bit) of the kernel's
    fp32 value is then decided.  The others are left out of the comparison, and there must be few of them (a condition on
    the test's operands, not a measurement: with randn operands the share is ~K * 2^-24)."""
    decided = f64(pre).abs() > f64(envelope)
    share = 1.0 - decided.double().mean().item()
    assert share < max_share, f"{share:.2e} of the pre-activations lie within the envelope of zero"
    return decided


def rounding_margin(value: Tensor, envelope: Tensor, max_share: float = 1e-3) -> Tuple[Tensor, float]:
    """the analogue of mask_margin for a value a kernel rounds to bf16 and never stores (the dX GEMM outputs in front of the chain's
    LayerNorm backward): where the fp64 value lies within ``envelope`` of a bf16 rounding boundary (the midpoint of two neighbours),
    the kernel's fp32 value may round to the other neighbour, one bf16 ulp away from rb(value).  Returns the per-element allowance --
    one ulp of the value's binade where the rounding is undecided, zero elsewhere -- and the undecided share, which must stay below
    ``max_share`` (a condition on the operands and the envelope, not a measurement of a kernel).
    Where the envelope is no longer small against the ulp (4 e >= ulp: a sum that cancels to almost nothing) the fp32 value v' may
    lie several ulps away: |rb(v') - rb(v)| <= |v' - v| + ulp(v') / 2 + ulp(v) / 2 with ulp(v') <= 2^-7 (|v| + e), hence < 2 (e + ulp)."""
    v, e = f64(value), f64(envelope)
    r = rb(v)
    ulp = 2.0 ** (torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 7)       # spacing of bf16 in the value's binade
    # distance to the nearest rounding boundary: the midpoints sit half an ulp from the rounded value
    dist = (ulp / 2 - (v - r).abs()).abs()
    undecided = dist <= e
    share = undecided.double().mean().item()
    assert share < max_share, f"{share:.2e} of the hidden values lie within the envelope of a bf16 rounding boundary"
    return torch.where(undecided, torch.where(4 * e < ulp, ulp, 2 * (e + ulp)), torch.zeros_like(ulp)), share


# --------------------------------------------------------------------------------------
# LayerNorm: fp64 reference and the envelope of an fp32 evaluation
# --------------------------------------------------------------------------------------
def layernorm_fp64(x: Tensor, w: Tensor, b: Tensor, eps: float = 1e-5):
    """y, mean, std, xhat of a row-wise LayerNorm in fp64 (mean / std [M, 1])"""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    std = (var + eps).sqrt()
    xhat = (xd - mean) / std
    return xhat * w.double() + b.double(), mean, std, xhat


def layernorm_envelope(mean: Tensor, std: Tensor, xhat: Tensor, w: Tensor) -> Tensor:
    """y = gamma * (x - mean) / std + beta in fp32.  The row mean carries one fp32 rounding of a number of size |mean|
    (2^-24 |mean|; the factor 4 covers the summation), x - mean one of its own (2^-24 |x - mean|, and |x - mean| / std = |xhat|), so
    xhat moves by at most 4 * 2^-24 * (|mean| / std + 1) * max|xhat| and y by |gamma| times that; what follows (rstd, the multiply-add)
    is a couple of fp32 ulps of the result: the 2^-23 |ref| term of the caller."""
    return 4 * 2.0 ** -24 * (mean.abs() / std + 1) * w.double().abs() * xhat.abs().amax(1, keepdim=True).clamp_min(2.0 ** -24)


def assert_layernorm_stats(mu: Tensor, rs: Tensor, x: Tensor, mean: Tensor, std: Tensor, xhat: Tensor, name: str = "") -> Tuple[float, float]:
    """the stored row statistics of an fp32 LayerNorm against layernorm_fp64 of the same rows; returns (mean, rstd) error / bound.
    mean: within 4 fp32 roundings of the size of the partial sums it is made of.  On rows with |mean| >> spread (the offset rows
    of tests/test_gpu_conditioning.py) that size is |mean| itself; in general no partial sum of x / C exceeds the row's mean |x|
    (>= |mean|, equal up to spread / |mean| on offset rows), which is what is used here -- a row whose mean happens to cancel
    to 1e-6 still carries the roundings of summands of size 1.  rstd: (mean error / std) relative, plus two fp32 ulps."""
    mu, rs = f64(mu).view(-1), f64(rs).view(-1)
    mean, std, amax = f64(mean).view(-1), f64(std).view(-1), f64(xhat).abs().amax(1)
    size = f64(x).abs().mean(1)
    out = []
    for what, err, bound in (("mean", (mu - mean).abs(), 4 * 2.0 ** -24 * size),
                             ("rstd", (rs * std - 1).abs(), 4 * 2.0 ** -24 * (mean.abs() / std + 1) * amax + 2.0 ** -22)):
        bad = ~(err <= bound)
        if bool(bad.any()):
            row = int(torch.where(bad, torch.nan_to_num(err / bound, nan=float("inf")), torch.zeros_like(err)).argmax())
            raise AssertionError(f"{name} {what}: {int(bad.sum())} of {err.numel()} rows outside the bound; worst row {row} (64-row block {row // 64}, "
                                 f"32-row tile {row // TILE}): error {err[row].item():.3g}, allowed {bound[row].item():.3g}")
        out.append((err / bound).max().item())
    return out[0], out[1]


def layernorm_model(x: Tensor, w: Tensor, b: Tensor, dy: Optional[Tensor] = None, dresid: Optional[Tensor] = None,
                    keep: Optional[Tensor] = None, p: float = 0.0, eps: float = 1e-5, dtype: torch.dtype = torch.float32) -> dict:
    """The LayerNorm kernels' own formulas (csrc/layernorm.hip) evaluated with torch on the CPU in ``dtype``: two-pass mean and
    variance, rstd = 1 / sqrt(var + eps), y = xhat * gamma + beta, and with ``dy``

        g = dy * gamma;  dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) (+ dresid);  gq = dx * keep / (1 - p)

    dtype = float32 is the model whose error against fp64 sets the per-row and per-column bounds of tests/test_gpu_layernorm.py
    (a reference-side number: every product, sum and square root rounded to fp32, no bf16 rounding -- the caller rounds where a
    kernel stores bf16); dtype = float64 is the same code as a reference, which tests/test_layernorm_cases_host.py holds against
    autograd.  Left to the caller's margin: the wave-shuffle summation order and ``rsqrtf`` against torch's order and ``sqrt``.
    Column sums are returned as their TERMS [M, C] (dgamma: dy * xhat, dbeta: dy, gbias: gq) so that a caller can sum any row
    range, in fp32 for the model and in fp64 for the reference."""
    t = lambda v: None if v is None else v.detach().cpu().to(dtype)
    x, w, b, dy, dresid, keep = t(x), t(w), t(b), t(dy), t(dresid), t(keep)
    C = x.shape[1]
    mean = x.sum(1, keepdim=True) / C
    d = x - mean
    rstd = 1.0 / ((d * d).sum(1, keepdim=True) / C + eps).sqrt()
    xhat = d * rstd
    out = dict(y=xhat * w + b, mean=mean, rstd=rstd, xhat=xhat)
    if dy is None:
        return out
    g = dy * w
    c1, c2 = g.sum(1, keepdim=True) / C, (g * xhat).sum(1, keepdim=True) / C
    dx = rstd * (g - c1 - xhat * c2)
    if dresid is not None:
        dx = dx + dresid
    gq = dx if keep is None else dx * keep * torch.tensor(1.0 / (1.0 - p), dtype=dtype)
    out.update(dx=dx, g=gq, dgamma_terms=dy * xhat, dbeta_terms=dy, gbias_terms=gq)
    return out


LN_MARGIN = 4.0            # the kernels' wave-shuffle summation order and rsqrtf against the model's torch order and sqrt


def layernorm_row_bound(model: Tensor, ref: Tensor, C: int, tol: float, cancels: bool = False) -> Tuple[float, float]:
    """(bound, model's worst row): LN_MARGIN x the worst row of the fp32 model against fp64, and never below the suite's
    whole-tensor tolerance ``tol`` -- except for the backward's outputs (``cancels``) at C < 32: there dx cancels almost
    entirely (it lies in the C - 2 dimensions orthogonal to the row's ones and xhat), the whole-tensor tolerance means nothing
    for it, and the model sets the bound alone."""
    m = rowwise_rel(model, ref, C).max().item()
    return (LN_MARGIN * m if cancels and C < 32 else max(tol, LN_MARGIN * m)), m


def layernorm_column_bound(model_sum: Tensor, ref_sum: Tensor, ref_terms: Tensor) -> Tuple[Tensor, float]:
    """per-column bound on a column sum of M terms: LN_MARGIN x (the model's worst column error / sum |term|) x sum |term| of
    the column itself; returns (bound [C], the model's worst ratio)."""
    mag = f64(ref_terms).abs().sum(0).clamp_min(1e-300)
    worst = ((f64(model_sum) - f64(ref_sum)).abs() / mag).max().item()
    return LN_MARGIN * worst * mag, worst


def single_rounding_envelope(value: Tensor, n: int) -> float:
    """an fp32 value that is itself within a few fp32 ulps of fp64 (a length-n reduction feeds it), rounded once:
    envelope = n * 2^-23 * max |value|"""
    return n * 2.0 ** -23 * f64(value).abs().max().item()


# --------------------------------------------------------------------------------------
# attention: fp64 reference, forward envelope, CPU model of the bf16 MFMA kernels' rounding points
# --------------------------------------------------------------------------------------
def _split(qkv: Tensor, B: int, T: int, NH: int, H: int) -> Tuple[Tensor, Tensor, Tensor]:
    q, k, v = f64(qkv).view(B, T, 3, NH, H).permute(2, 0, 3, 1, 4)          # each (B, NH, T, H)
    return q, k, v


def _pack(x: Tensor) -> Tensor:
    B, NH, T, H = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, NH * H)


def attention_fp64(qkv: Tensor, dout: Optional[Tensor], B: int, T: int, NH: int, H: int, keep: Optional[Tensor] = None, p: float = 0.0,
                   model=False, scale: Optional[float] = None):
    """Causal attention over packed qkv [B*T, 3*NH*H] in fp64, written out by hand (no autograd) so that the same code serves
    as reference (model=False) and as the rounding model of the bf16 MFMA kernels (model=True):

      P = softmax(mask(q k^T * scale));  Pd = P * keep / (1 - p);  out = Pd v
      delta = rowsum(dout * out);  dPd = dout v^T;  dS = P * (dPd * keep / (1 - p) - delta)
      dv = Pd^T dout;  dq = dS k * scale;  dk = dS^T q * scale

    model=True rounds to bf16 exactly where the kernels store bf16: Pd before Pd v and Pd^T dout, out, dS before both of its
    products, the three gradients; delta is taken from the ROUNDED out (the backward reads the forward's stored output).
    Left out of the model, covered by the caller's margin: fp32 accumulation order, the hardware exp2, the kernels rounding
    the unnormalised exponentials and applying 1 / (rowsum * (1 - p)) to the finished row.
    model="fp32" is the counterpart for the fp32 kernels: the same formulas evaluated in torch float32 throughout (every
    product, sum and exponential rounded to fp32; delta from the fp32 out), no bf16 rounding.

    Returns dict(out, lse, P, Pd, v [, dq, dk, dv, dqkv; reference only: dq_mag, dk_mag, dv_mag]), out / dqkv packed like the
    kernels' tensors."""
    wd = torch.float32 if model == "fp32" else torch.float64
    q, k, v = (t.to(wd) for t in _split(qkv, B, T, NH, H))
    scale = H ** -0.5 if scale is None else scale
    r = (lambda x: rb(x)) if model in (True, "bf16") else (lambda x: x)
    keep = None if keep is None else f64(keep).to(wd)
    s = q @ k.transpose(-2, -1) * scale
    tril = torch.tril(torch.ones(T, T, dtype=torch.bool))
    s = s.masked_fill(~tril, float("-inf"))
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse.unsqueeze(-1))
    Pd = P if keep is None else P * keep / (1.0 - p)
    Pm = r(Pd).to(wd)
    out = r(Pm @ v).to(wd)
    res = dict(out=_pack(out).double(), lse=lse.double(), P=P, Pd=Pd, v=v)
    if dout is None:
        return res
    do = f64(dout).view(B, T, NH, H).permute(0, 2, 1, 3).to(wd)
    delta = (do * out).sum(-1, keepdim=True)
    dPd = do @ v.transpose(-2, -1)
    dP = dPd if keep is None else dPd * keep / (1.0 - p)
    dS = r(P * (dP - delta)).to(wd)
    dv = r(Pm.transpose(-2, -1) @ do)
    dq = r(dS @ k * scale)
    dk = r(dS.transpose(-2, -1) @ q * scale)
    res.update(dq=_pack(dq).double(), dk=_pack(dk).double(), dv=_pack(dv).double())
    if not model:                                                     # the same contractions over absolute values (structured_floor)
        res.update(dq_mag=_pack(dS.abs() @ k.abs() * scale), dk_mag=_pack(dS.abs().transpose(-2, -1) @ q.abs() * scale),
                   dv_mag=_pack(Pm.abs().transpose(-2, -1) @ do.abs()))
    res["dqkv"] = torch.stack([res["dq"], res["dk"], res["dv"]], 1).reshape(B * T, 3 * NH * H)
    return res


def attention_fwd_envelope(ref: dict) -> Tensor:
    """bf16 MFMA forward: each probability enters the P V MFMA as bf16 (2^-8 relative at most), so the sum moves by at most
    2^-8 * (Pd |V|); the output's own rounding is the ``ulps`` term of assert_within_rounding.  Packed like ``out``."""
    return _pack(ref["Pd"] @ ref["v"].abs()) * BF16_RN


BWD_MARGIN = 3.0
BWD_WINDOW = 16


def attention_bwd_bounds(ref: dict, model: dict, H: int) -> dict:
    """per gradient third: BWD_MARGIN x the model's worst (row, head) against the fp64 reference"""
    return {n: BWD_MARGIN * rowwise_rel(model[n], ref[n], H).max().item() for n in ("dq", "dk", "dv")}


def structured_floor(ref: dict, n: str, H: int) -> float:
    """Denominator floor for gradients of structured operands, where the median group is no scale: near one-hot rows leave dq
    zero up to fp32 summation order in most rows (median 3e-6) and 58 in a few; identical keys make dq vanish identically
    (softmax-gradient rows sum to zero).  The larger of the RMS group norm of the reference and 2^-8 x the RMS group norm of
    the same contraction over absolute values: what cancels to below one bf16 rounding of its summands is noise for the
    reference too."""
    rms = lambda x: f64(x).reshape(-1, H).norm(dim=1).square().mean().sqrt().item()
    return max(rms(ref[n]), BF16_RN * rms(ref[n + "_mag"]))


def attention_bwd_bounds_by_position(ref: dict, model: dict, B: int, T: int, NH: int, H: int, at_least: float = 0.0,
                                     floors: Optional[dict] = None) -> dict:
    """The same rule resolved along the sequence: per group, BWD_MARGIN x the model's worst group among all (batch, head)
    pairs at positions within BWD_WINDOW rows of the group's own.  Never above attention_bwd_bounds, usually far below.

    Why: the model's worst dq groups are the first few query rows.  There dq is a near-cancellation (row 0: exactly zero in
    fp64) and delta = rowsum(dout * out) is taken from the bf16-ROUNDED out, as the kernels take it, so the row carries an
    error of 2^-9 |dout||out| against a denominator at its floor: 0.1 .. 0.4 per group where every later row has ~4e-3.
    One global maximum would then admit a zeroed (row, head) of dq anywhere.  A row's error there is one random scalar
    (delta's) times a fixed vector, so a group is not compared with the model's error of the SAME group (either may be
    near zero by chance) but with the largest of >= BWD_WINDOW + 1 rows x B x NH model groups around it.

    ``at_least``: a floor under every bound, the suite's fp32 tolerance where it is used.  Structured operands make the
    model's error EXACTLY zero in whole groups (a one-hot row: dP - delta cancels exactly in fp64) where a kernel, bf16 or
    fp32, is left with the fp32 summation-order difference between its two dot products.  The fp32 kernels (model="fp32"): ordinary rows are judged at the suite's fp32 tolerance, which covers the
    kernels' sequential length-T sums that torch's blocked fp32 sums understate; the model raises the bound only where
    the cancellation above does (fp32: 2^-24 instead of 2^-9, the same rows)."""
    out = {}
    for n in ("dq", "dk", "dv"):
        e = rowwise_rel(model[n], ref[n], H, floors[n] if floors else 0.0).view(B, T, NH).amax(dim=(0, 2))      # worst per position
        pad = torch.nn.functional.pad(e.view(1, 1, T), (BWD_WINDOW, BWD_WINDOW), value=0.0)
        win = torch.nn.functional.max_pool1d(pad, 2 * BWD_WINDOW + 1, 1).view(T)
        out[n] = (BWD_MARGIN * win).clamp_min(at_least).view(1, T, 1).expand(B, T, NH).reshape(-1)
    return out


def assert_rowwise_each(got: Tensor, ref: Tensor, group: int, bounds: Tensor, name: str = "", T: Optional[int] = None,
                        floor: float = 0.0) -> float:
    """every group's rowwise_rel below its own bound; returns the largest ratio error / bound"""
    e = rowwise_rel(got, ref, group, floor)
    bad = ~(e <= bounds)                                  # (a group that is exactly zero in reference, model and kernel passes)
    ratio = e / bounds.clamp_min(1e-300)
    if bool(bad.any()):
        worst = int(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax())
        per_row = max(f64(ref).shape[-1] // group, 1)
        raise AssertionError(f"{name}: {int(bad.sum())} of {e.numel()} groups over their bound; worst {e[worst].item():.3e} >= "
                             f"{bounds[worst].item():.3e} at {describe_group(worst, per_row, T)}")
    return ratio.max().item()


# --------------------------------------------------------------------------------------
# decode attention: one query (position t) against a K/V cache kept in the training layout
# --------------------------------------------------------------------------------------
def decode_attention_fp64(cache: Tensor, t: int, B: int, Tcap: int, NH: int, H: int, scale: Optional[float] = None,
                          row: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """out[b, h] = softmax(q_t . K[0..t]^T * scale) . V[0..t] over a cache [B, Tcap, 3*NH*H] (row = position, q | k | v thirds,
    heads inside a third).  ``row`` [B, 3*NH*H]: row t is replaced by it first (the append form: the new token's q/k/v arrive
    in a staging row).  Rows > t are never touched (they may hold NaN).  Returns out [B, NH*H] and P [B, NH, t+1], fp64."""
    assert tuple(cache.shape) == (B, Tcap, 3 * NH * H) and 0 <= t < Tcap, (tuple(cache.shape), t)
    c = cache.detach().cpu().reshape(B, Tcap, 3, NH, H)
    n = t + 1 if row is None else t                                       # (the thirds are converted one by one: 50 MB caches)
    q, k, v = f64(c[:, t, 0]), f64(c[:, :n, 1]), f64(c[:, :n, 2])         # (B, NH, H), (B, n, NH, H) twice
    if row is not None:
        r = f64(row).reshape(B, 3, NH, H)
        q, k, v = r[:, 0], torch.cat([k, r[:, 1:2]], 1), torch.cat([v, r[:, 2:3]], 1)
    scale = H ** -0.5 if scale is None else scale
    P = torch.softmax(torch.einsum("bhd,bjhd->bhj", q, k) * scale, -1)
    return torch.einsum("bhj,bjhd->bhd", P, v).reshape(B, NH * H), P


def spotlight_decode_inputs(B: int, Tcap: int, NH: int, H: int, t: int, j_star: int, seed: int, dtype: torch.dtype) -> Tensor:
    """A randn cache [B, Tcap, 3*NH*H] in ``dtype`` whose key j_star holds about half of query t's probability in every (b, h):
    k[b, j_star, h] = c * q / |q| with c solved in fp64 so that its score equals the log-sum-exp of the other keys' scores.
    At t = 8191 a randn key holds ~1e-4 of the mass and a kernel that drops it (or reads a stale row in its place) stays inside
    a bf16 bound; with the spotlight on that key the same kernel is wrong by O(1).
    The condition 0.25 <= P[b, h, j_star] <= 0.75 is asserted on the fp64 reference of the ROUNDED inputs: a condition on the
    operands, not a measurement."""
    assert 1 <= t < Tcap and 0 <= j_star <= t, (t, j_star, Tcap)
    g = torch.Generator().manual_seed(seed)
    cache = torch.randn((B, Tcap, 3 * NH * H), generator=g).to(dtype)
    c = cache.view(B, Tcap, 3, NH, H)
    scale = H ** -0.5
    q = f64(c[:, t, 0])                                                   # (B, NH, H)
    s = torch.einsum("bhd,bjhd->bhj", q, f64(c[:, :t + 1, 1])) * scale
    s[:, :, j_star] = float("-inf")
    qn = q.norm(dim=-1, keepdim=True)
    key = q / qn * (torch.logsumexp(s, -1, keepdim=True) / (qn * scale))  # score of the key = lse of the others
    cache.view(B, Tcap, 3, NH, H)[:, j_star, 1] = key.to(dtype)
    P = decode_attention_fp64(cache, t, B, Tcap, NH, H)[1][:, :, j_star]
    assert 0.25 <= P.min().item() and P.max().item() <= 0.75, (P.min().item(), P.max().item())
    return cache


DECODE_TOL_FP32 = 2e-5                     # the suite's fp32 attention-forward tolerance (tests/test_gpu_ops.py)
# bf16: the decode kernels compute in fp32 and round only the stored output, which moves every element by at most 2^-8 |x|,
# hence a (b, head) group by at most 2^-8 of its norm; the fp32 arithmetic in front of it gets the fp32 tolerance
DECODE_TOL_BF16 = BF16_RN + DECODE_TOL_FP32


def assert_decode_output(got: Tensor, ref: Tensor, H: int, dtype: torch.dtype, name: str = "") -> float:
    """a decode-attention output [B, NH*H] against decode_attention_fp64: finite, and every (b, head) group within the bound
    of its dtype.  Returns the worst group."""
    if not bool(torch.isfinite(f64(got)).all()):
        raise AssertionError(f"{name}: {int((~torch.isfinite(f64(got))).sum())} non-finite elements")
    return assert_rowwise(got, ref, H, DECODE_TOL_BF16 if dtype == torch.bfloat16 else DECODE_TOL_FP32, name)


# --------------------------------------------------------------------------------------
# planted defects (host tensors only): what the localized checks must catch
# --------------------------------------------------------------------------------------
def plant(x: Tensor, kind: str, group: int) -> Tensor:
    """a copy of the 2-D tensor x with one localized defect; ``group`` = elements per (row, head)"""
    y = x.clone()
    M, N = y.shape
    r0 = min(M - 1, (M // 2) // TILE * TILE + TILE - 1)                     # last row of a 32-row tile in the middle
    c0 = (N // group // 2) * group
    if kind == "zero_group":
        y[r0, c0:c0 + group] = 0
    elif kind == "scale_row":
        y[r0, c0:c0 + group] *= 1.3
    elif kind == "chunk_from_neighbour":
        y[r0, c0:c0 + 8] = x[r0, c0 + 8:c0 + 16]
    elif kind == "swap_rows_at_tile_edge":
        y[r0, c0:c0 + group] = x[r0 + 1, c0:c0 + group]
        y[r0 + 1, c0:c0 + group] = x[r0, c0:c0 + group]
    elif kind == "zero_last_row":
        y[M - 1, N - group:] = 0
    else:
        raise ValueError(kind)
    return y


DEFECTS: Sequence[str] = ("zero_group", "scale_row", "chunk_from_neighbour", "swap_rows_at_tile_edge", "zero_last_row")
