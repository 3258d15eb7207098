"""The block-chain kernels (csrc/chain.hip, csrc/chain_bwd.hip) stage by stage in fp64 -- TEST INFRASTRUCTURE (CPU).

Three things live here, shared by tests/test_gpu_chain_parity.py (the launch on the GPU) and tests/test_parity_host.py (a CPU
stand-in with planted defects):

  * the operand recipe (o ~ N(0, 1), x ~ 2 N(0, 1), weights N(0, 1 / K), biases 0.1 N, gamma = 1 + 0.1 N) and the host keep masks;
  * ``check_fwd`` / ``check_bwd``: every stage of a launch against fp64 evaluated on the launch's OWN stored input of that stage
    (never against another kernel), inside the derived envelopes of oracle/parity.py.  A stale resident operand, a ring slot
    refilled too early or a read in front of its store's acknowledgement shows at the stage that consumed the bad operand;
  * ``fwd_standin`` / ``bwd_standin``: the fp64 chain with a rounding at each of the kernel's store points, optionally with one
    planted defect.

All tensors are host tensors; ``got`` maps the names of ops.block_chain_fwd / ops.block_chain_bwd to what the launch stored."""
import functools
import re

import torch

from oracle import parity as P
from oracle import rng_ref

C = 384
ROWS = 64                                   # rows per block: one workgroup owns a block and walks the whole chain for it
bf = torch.bfloat16
SEED, STEP = 99, 5
SITE_PROJ, SITE_FFN = rng_ref.site_proj(2), rng_ref.site_ffn(2)
f64 = P.f64


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
def fwd_operands(M, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    op = dict(o=rn(M, C).to(bf), x=rn(M, C, sc=2.0), f_in=rn(M, 4 * C).clamp_min(0).to(bf))
    op.update({k: v.to(bf) for k, v in dict(wproj=rn(C, C, sc=C ** -0.5), w1=rn(4 * C, C, sc=C ** -0.5), w2=rn(C, 4 * C, sc=(4 * C) ** -0.5),
                                            wqkv=rn(3 * C, C, sc=C ** -0.5)).items()})
    op.update(bproj=rn(C, sc=0.1), b1=rn(4 * C, sc=0.1), b2=rn(C, sc=0.1), ln2w=1 + rn(C, sc=0.1), ln2b=rn(C, sc=0.1), ln1w=1 + rn(C, sc=0.1),
              ln1b=rn(C, sc=0.1))
    return op


WEIGHTS = ("wproj", "w1", "w2", "wqkv")
VECTORS = ("bproj", "b1", "b2", "ln2w", "ln2b", "ln1w", "ln1b")


@functools.lru_cache(maxsize=4)
def keep_scales(M, p, site_a=SITE_PROJ, site_b=SITE_FFN):
    """keep / (1 - p) of the two dropout sites as fp64 [M, C] (None, None at p = 0): computed once per shape, never modified"""
    if p <= 0:
        return None, None
    return tuple(torch.from_numpy(rng_ref.keep_mask(SEED, STEP, s, p, M * C).reshape(M, C)).double() / (1.0 - p) for s in (site_a, site_b))


def _parts(mode):
    return dict(proj=mode in (0, 1, 3), ffn1=mode in (0, 1), ffn2=mode in (0, 1, 4), ln1=mode in (0, 2, 4), qkv=mode in (0, 2))


def _located(stage, grid, fn):
    """run one stage's assertion; on failure name the stage and the block / workgroup / round of the worst element"""
    try:
        return fn()
    except AssertionError as e:
        msg = f"stage {stage}: {e}"
        m = re.search(r"worst (?:at \(|row )(\d+)", str(e))
        if m:
            blk = int(m.group(1)) // ROWS
            msg += f" [64-row block {blk}" + (f": workgroup {blk % grid}, round {blk // grid} of a grid of {grid}]" if grid else "]")
        raise AssertionError(msg) from None


# ---------------------------------------------------------------------------------------------------------------------
# forward: stage checks
# ---------------------------------------------------------------------------------------------------------------------
def check_bits(mask, f_got, pre, decided):
    """mask: the sign bits as their consumer reads them (exact 0 / 1 per element of the [M, 4C] hidden block)"""
    m = f64(mask)
    if not bool(((m == 0) | (m == 1)).all()):
        raise AssertionError("the probe returned values other than 0 / 1")
    m = m > 0.5

    def first(bad, what):
        if bool(bad.any()):
            r, c = (int(v[0]) for v in torch.nonzero(bad, as_tuple=True))
            raise AssertionError(f"{int(bad.sum())} of {bad.numel()} sign bits differ from {what}; worst at ({r}, {c}) (8-element chunk {c // 8} of row {r})")
    first(m != (f64(f_got) > 0), "(stored f > 0)")                       # every element: the bit and the value come from one register
    first((m != (f64(pre) > 0)) & decided, "the sign of the fp64 pre-activation")
    return 1.0 - decided.double().mean().item()


def _check_ln(use, grid, tag, pre, h, mu, rs, w, b):
    ref, mean, std, xhat = P.layernorm_fp64(pre, w, b)
    env = P.layernorm_envelope(mean, std, xhat, w)
    use[f"mean{tag}"], use[f"rstd{tag}"] = _located(f"mean{tag}/rstd{tag}", grid, lambda: P.assert_layernorm_stats(mu, rs, pre, mean, std, xhat, f"LayerNorm {tag}"))
    use[f"h{tag}"] = _located(f"h{tag}", grid, lambda: P.assert_within_rounding(h, ref, env + 2.0 ** -23 * ref.abs(), 1, f"h{tag}"))


def check_fwd(got, op, mode, p, mask=None, grid=0):
    """every stage the launch of ``mode`` stores against fp64 on its own stored input; returns {stage: error / bound}.
    ``mask``: the sign bits read through their consumer (modes 0 / 1).  ``grid``: workgroups of the launch, for the messages."""
    M = op["x"].shape[0]
    has = _parts(mode)
    kp, kf = keep_scales(M, p)
    use = {}
    if has["proj"]:
        acc = f64(op["o"]) @ f64(op["wproj"]).T + f64(op["bproj"])
        ref = f64(op["x"]) + (acc if kp is None else kp * acc)
        env = P.gemm_envelope(op["o"], op["wproj"], C, op["bproj"], op["x"], keep_scale=kp) + 2.0 ** -23 * ref.abs()
        use["x1"] = _located("x1", grid, lambda: P.assert_within_rounding(got["x1"], ref, env, 0, "x1"))
        _check_ln(use, grid, "2", got["x1"], got["h2"], got["mean2"], got["rstd2"], op["ln2w"], op["ln2b"])
    if has["ffn1"]:
        pre = f64(got["h2"]) @ f64(op["w1"]).T + f64(op["b1"])
        env = P.gemm_envelope(got["h2"], op["w1"], C, op["b1"])           # (the bias term |b1| K 2^-24 is part of it)
        decided = P.mask_margin(pre, env)
        use["f"] = _located("f", grid, lambda: P.assert_within_rounding(got["f"], pre.clamp_min(0), env, 1, "f", where=decided))
        use["bits undecided"] = _located("bits", grid, lambda: check_bits(mask, got["f"], pre, decided))
        del pre, env, decided
    if has["ffn2"]:
        fin, x1 = (got["f"], got["x1"]) if has["ffn1"] else (op["f_in"], op["x"])
        acc = f64(fin) @ f64(op["w2"]).T + f64(op["b2"])
        ref = f64(x1) + (acc if kf is None else kf * acc)
        env = P.gemm_envelope(fin, op["w2"], 4 * C, op["b2"], x1, keep_scale=kf) + 2.0 ** -23 * ref.abs()
        use["x2"] = _located("x2", grid, lambda: P.assert_within_rounding(got["x2"], ref, env, 1 if mode == 1 else 0, "x2"))
    if has["ln1"]:
        _check_ln(use, grid, "1", op["x"] if mode == 2 else got["x2"], got["h1"], got["mean1"], got["rstd1"], op["ln1w"], op["ln1b"])
    if has["qkv"]:
        ref = f64(got["h1"]) @ f64(op["wqkv"]).T
        use["qkv"] = _located("qkv", grid, lambda: P.assert_within_rounding(got["qkv"], ref, P.gemm_envelope(got["h1"], op["wqkv"], C), 1, "qkv"))
    return use


# ---------------------------------------------------------------------------------------------------------------------
# forward: the CPU stand-in (fp64 arithmetic, one rounding at each store point of the kernel) and its planted defects
# ---------------------------------------------------------------------------------------------------------------------
FWD_DEFECTS = ("f_chunk_from_neighbour", "h2_rows_swapped_at_32_row_edge", "stale_resident_h2", "stats_from_three_partials",
               "x2_wave_column_without_inv_keep", "decided_sign_bit_flipped", "qkv_last_row_zero")
# the stage whose check must refuse each of them
FWD_DEFECT_STAGE = dict(f_chunk_from_neighbour="stage f", h2_rows_swapped_at_32_row_edge="stage h2", stale_resident_h2="stage f",
                        stats_from_three_partials="stage mean2/rstd2", x2_wave_column_without_inv_keep="stage x2",
                        decided_sign_bit_flipped="stage bits", qkv_last_row_zero="stage qkv")


def _ln_store(pre, w, b, three_partials_block=None):
    y, mean, std, xhat = P.layernorm_fp64(pre, w, b)
    mean, rstd = mean.view(-1).clone(), (1.0 / std).view(-1)
    if three_partials_block is not None:                                  # the fourth 96-column partial never reached the exchange
        r = slice(three_partials_block * ROWS, (three_partials_block + 1) * ROWS)
        part = pre[r, :288].double()
        m = part.mean(1)
        mean[r] = m
        rstd[r] = 1.0 / (((part - m[:, None]) ** 2).mean(1) + 1e-5).sqrt()
        y = y.clone()
        y[r] = (pre[r].double() - m[:, None]) * rstd[r, None] * w.double() + b.double()
    return P.rb(y).to(bf), mean.float(), rstd.float()


def fwd_standin(op, mode, p, defect=None, cus=2):
    """what a correct launch stores (fp32 accumulation stood in for by fp64 rounded once), plus "mask": the sign bits as 0 / 1.
    ``defect``: one of FWD_DEFECTS, planted where the kernel would make it (block 1 of workgroup 1 unless the defect says otherwise;
    ``cus``: the grid the stale-operand defect assumes).  Everything downstream of a defect is computed from the damaged value, as
    the kernel would: only the stage that consumed or produced it may fail."""
    M = op["x"].shape[0]
    has = _parts(mode)
    kp, kf = keep_scales(M, p)
    blk = min(cus + 1, M // ROWS - 1)                                     # a block of the second round
    rows = slice(blk * ROWS, (blk + 1) * ROWS)
    out = {}
    if has["proj"]:
        acc = f64(op["o"]) @ f64(op["wproj"]).T + f64(op["bproj"])
        out["x1"] = (f64(op["x"]) + (acc if kp is None else kp * acc)).float()
        out["h2"], out["mean2"], out["rstd2"] = _ln_store(out["x1"], op["ln2w"], op["ln2b"], blk if defect == "stats_from_three_partials" else None)
        if defect == "h2_rows_swapped_at_32_row_edge":
            r = blk * ROWS + 31
            out["h2"][[r, r + 1]] = out["h2"][[r + 1, r]]
    if has["ffn1"]:
        a = f64(out["h2"])
        if defect == "stale_resident_h2":                                 # the image the block `cus` positions earlier (same workgroup) left in LDS
            a = a.clone()
            a[rows] = f64(out["h2"])[(blk - cus) * ROWS:(blk - cus + 1) * ROWS]
        v = (a @ f64(op["w1"]).T + f64(op["b1"])).float()
        out["f"] = v.clamp_min(0).to(bf)
        out["mask"] = (v > 0).float()
        if defect == "f_chunk_from_neighbour":
            r, c = blk * ROWS + 31, 2 * C + 96
            out["f"][r, c:c + 8] = out["f"][r, c + 8:c + 16].clone()
            out["mask"][r, c:c + 8] = out["mask"][r, c + 8:c + 16].clone()
        if defect == "decided_sign_bit_flipped":
            pre = f64(out["h2"]) @ f64(op["w1"]).T + f64(op["b1"])
            decided = pre.abs() > P.gemm_envelope(out["h2"], op["w1"], C, op["b1"])
            r = blk * ROWS + 17
            c = int(torch.nonzero(decided[r] & (pre[r] < 0))[0])
            out["mask"][r, c] = 1.0
    if has["ffn2"]:
        fin, x1 = (out["f"], out["x1"]) if has["ffn1"] else (op["f_in"], op["x"])
        acc = f64(fin) @ f64(op["w2"]).T + f64(op["b2"])
        sc = kf
        if defect == "x2_wave_column_without_inv_keep":
            sc = kf.clone()
            sc[rows, 96:192] *= 1.0 - p
        x2 = f64(x1) + (acc if sc is None else sc * acc)
        out["x2"] = x2.float().to(bf) if mode == 1 else x2.float()
    if has["ln1"]:
        out["h1"], out["mean1"], out["rstd1"] = _ln_store(op["x"] if mode == 2 else out["x2"], op["ln1w"], op["ln1b"])
    if has["qkv"]:
        out["qkv"] = (f64(out["h1"]) @ f64(op["wqkv"]).T).float().to(bf)
        if defect == "qkv_last_row_zero":
            out["qkv"][M - 1] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# backward (dg_block_chain_bwd): operands, stage checks, stand-in
# ---------------------------------------------------------------------------------------------------------------------
PART_STRIDE = 12 * C
# columns of the partial buffer: name -> (first column, width)
PART_COLS = dict(dln1w=(0, C), dln1b=(C, C), gbias1=(2 * C, C), dln2w=(3 * C, C), dln2b=(4 * C, C), gbias2=(5 * C, C), db1=(8 * C, 4 * C))


def bwd_operands(M, seed):
    """the recipe of test_block_chain_bwd_kernel_equals_the_launches_it_replaces; the forward statistics are those of x / x1 in
    fp64, stored as fp32 (inputs of the launch); "mask": a ReLU pattern for the host stand-in (the GPU test makes sign bits)"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    op = {k: v.to(bf) for k, v in dict(wqkvT=rn(C, 3 * C, sc=(3 * C) ** -0.5), w2T=rn(4 * C, C, sc=C ** -0.5), w1T=rn(C, 4 * C, sc=(4 * C) ** -0.5),
                                       wprojT=rn(C, C, sc=C ** -0.5), dqkv=rn(M, 3 * C), dresid=rn(M, C), g_in=rn(M, C)).items()}
    op.update(x=rn(M, C, sc=2.0), x1=rn(M, C, sc=2.0), ln1w=1 + rn(C, sc=0.1), ln2w=1 + rn(C, sc=0.1))
    for n, src in (("1", "x"), ("2", "x1")):
        _, mean, std, _ = P.layernorm_fp64(op[src], torch.ones(C), torch.zeros(C))
        op["mean" + n], op["rstd" + n] = mean.view(-1).float(), (1.0 / std).view(-1).float()
    op["mask"] = (torch.rand(M, 4 * C, generator=g) < 0.5).float()
    # operands of the launch that makes the sign bits on the GPU (a ReLU GEMM on operands of its own)
    op["bits_a"], op["bits_w"] = rn(M, C).to(bf), rn(4 * C, C, sc=C ** -0.5).to(bf)
    return op


BWD_WEIGHTS = ("wqkvT", "w2T", "w1T", "wprojT")


def _ln_bwd_fp64(dh, x, mean, rstd, gamma, dresid, xh_round=False):
    """dx = rstd (t - mean_c(t) - xh mean_c(t xh)) + dresid with t = dh gamma, xh = (x - mean) rstd, on the launch's stored
    statistics.  xh_round: x-hat crosses the kernel's row-sum exchange as bf16 (the stand-in rounds it there)."""
    rs = f64(rstd).view(-1, 1)
    xh = (f64(x) - f64(mean).view(-1, 1)) * rs
    t = f64(dh) * f64(gamma)
    c1, c2 = t.mean(1, keepdim=True), (t * xh).mean(1, keepdim=True)
    dx = rs * (t - c1 - (P.rb(xh) if xh_round else xh) * c2) + f64(dresid)
    return dx, xh, c2


def _check_partial(parts, name, terms, allow, label):
    """a column-sum partial of the launch against fp64 sums of the same terms [M, w]: each partial row (row 2 * block + wave row of
    the buffer = the sum over that wave row's 32 rows), then their total.  Bound: the fp32 summation envelope n 2^-24 sum |term| over
    the n rows summed, plus ``allow`` [M, w], what the kernel's own summands may legitimately differ by.  Returns the largest
    error / bound."""
    a, w = PART_COLS[name]
    M = terms.shape[0]
    got = f64(parts)[:, a:a + w]
    assert got.shape[0] == M // 32, (got.shape, M)
    by_row = lambda t: t.view(M // 32, 32, w).sum(1)
    worst = 0.0
    for what, g, ref, bound in ((f"{label}, partial rows", got, by_row(terms), 32 * 2.0 ** -24 * by_row(terms.abs()) + by_row(allow)),
                                (f"{label}, total", got.sum(0, keepdim=True), terms.sum(0, keepdim=True),
                                 M * 2.0 ** -24 * terms.abs().sum(0, keepdim=True) + allow.sum(0, keepdim=True))):
        err = (g - ref).abs()
        bad = ~(err <= bound)
        if bool(bad.any()):
            flat = int(torch.where(bad, torch.nan_to_num(err / bound, nan=float("inf")), torch.zeros_like(err)).reshape(-1).argmax())
            r, c = divmod(flat, w)
            raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} sums outside the bound; worst at partial row {r} (64-row block {r // 2}, wave row "
                                 f"{r % 2}), column {c} (96-column wave column {(c % C) // 96}): got {g[r, c].item():.6g}, ref {ref[r, c].item():.6g}, "
                                 f"allowed {bound[r, c].item():.3g}")
        ok = bound > 0
        worst = max(worst, (err[ok] / bound[ok]).max().item() if bool(ok.any()) else 0.0)
    return worst


def _check_ln_bwd(use, tag, got, parts, dh_exact, dh_env, x, mean, rstd, gamma, dresid, scale, has_bias, max_share):
    """one LayerNorm-backward half: dx / g per row, dgamma / dbeta / bias partial per column.  dh_exact: the fp64 dX GEMM of the
    stored operand; the kernel rounds its fp32 value to bf16 in registers and never stores it, so the reference is rb(dh_exact)."""
    dh = P.rb(dh_exact)
    dx, xh, c2 = _ln_bwd_fp64(dh, x, mean, rstd, gamma, dresid)
    g = dx if scale is None else scale * dx
    rs, gmax = f64(rstd).view(-1), f64(gamma).abs().max().item()
    # Per row.  The output's own bf16 rounding moves a row by at most 2^-8 of its norm.  The hidden operand: dx is rstd times a
    # projection of t = gamma dh (I - 11^T / C - xh xh^T / C has norm 1), so if EVERY element of dh were one bf16 ulp off (2^-8 |dh|:
    # the rounding is undecided where the fp32 value straddles a boundary) the row would move by at most rstd max|gamma| 2^-8 |dh row|.
    # (x-hat's own bf16 rounding in pass 2, 2^-9 |xh| |c2| rstd per element with |c2| ~ |t| / sqrt(C), stays far inside that term.)
    hidden = rs * gmax * P.BF16_RN * dh.norm(dim=1)
    for name, ref, k in (("dx" + tag, dx, 1.0), ("g" + tag, g, 1.0 if scale is None else scale.max().item())):
        den = ref.norm(dim=1)
        den = den.clamp_min(max(0.1 * den.median().item(), 1e-300))      # rowwise_rel's denominators
        bounds = P.BF16_RN + k * hidden / den
        # (a condition on the operands: the bound stays near 1e-2, where a lost residual or 1 / (1 - p) moves a row by 20 .. 90 % and a
        # lost mean term, the smallest of the three on zero-mean operands, by 2 %)
        assert bounds.max().item() < 3e-2, (name, bounds.max().item())
        use[name] = _located(name, 0, lambda: P.assert_rowwise_each(got[name], ref, C, bounds, name))
    # Per column.  Where dh's rounding is undecided (rounding_margin) the kernel's summand may be one ulp of dh away: allow[r, c]
    # times the summand's coefficient.
    allow, share = P.rounding_margin(dh_exact, dh_env, max_share)
    use["dln%sw" % tag] = _check_partial(parts, "dln%sw" % tag, dh * xh, allow * xh.abs(), "dgamma" + tag)
    use["dln%sb" % tag] = _check_partial(parts, "dln%sb" % tag, dh, allow, "dbeta" + tag)
    if has_bias:
        # the bias partial sums the fp32 g in front of its rounding.  An undecided dh element moves its own g by rstd |gamma| ulp and,
        # through the two row means, every g of its row by rstd (a1 + |xh| a2), a1 = mean_c(|gamma| allow), a2 = mean_c(|gamma| allow |xh|);
        # x-hat enters pass 2 as bf16: rstd 2^-8 |xh| |c2|.  All times keep / (1 - p).
        ga = f64(gamma).abs() * allow
        a1, a2 = ga.mean(1, keepdim=True), (ga * xh.abs()).mean(1, keepdim=True)
        moved = rs.view(-1, 1) * (ga + a1 + xh.abs() * a2 + P.BF16_RN * xh.abs() * c2.abs())
        if scale is not None:
            moved = moved * scale
        use["gbias" + tag] = _check_partial(parts, "gbias" + tag, g, moved, "bias partial " + tag)
    use["undecided" + tag] = share


def check_bwd(got, parts, op, mode, p, mask, max_share=1.0):
    """got: dx1 / g1 / df / dx2 / g2 / dout of the launch, parts: its partial buffer [2 M / 64, PART_STRIDE]; mask: the sign bits as
    0 / 1.  Returns {stage: error / bound}.
    max_share: rounding_margin's cap on the hidden elements whose bf16 rounding the GEMM envelope leaves undecided.  No "few of
    them" condition can hold here: K 2^-24 sum |a||b| is the worst case over every summation order, at K = 3C / 4C about 1.5e-3 against
    a bf16 spacing of 2^-8 |dh| ~ 3e-3, and 0.72 .. 0.76 of the elements are undecided on the fp64 reference alone (recorded as
    "undecided1" / "undecided2").  The allowance therefore counts almost every element, and what keeps it meaningful is its size: one
    ulp is at most 2^-7 of the summand, so a partial sum's bound stays below 1 % of the absolute sum of its terms -- a lost row of a
    32-row partial or a lost wave-row partial of a column is refused (tests/test_parity_host.py), drift of a few ulps is not seen."""
    M = op["x"].shape[0]
    has_q, has_2 = mode in (0, 2), mode in (0, 1)
    k1, k2 = keep_scales(M, p, SITE_FFN, SITE_PROJ)                      # site_ffn_below, site_proj
    use = {}
    if has_q:
        dh = f64(op["dqkv"]) @ f64(op["wqkvT"]).T
        _check_ln_bwd(use, "1", got, parts, dh, P.gemm_envelope(op["dqkv"], op["wqkvT"], 3 * C), op["x"], op["mean1"], op["rstd1"], op["ln1w"],
                      op["dresid"], k1 if mode == 0 else None, mode == 0, max_share)
    if has_2:
        a = got["g1"] if mode == 0 else op["g_in"]
        m = f64(mask)
        ref = (f64(a) @ f64(op["w2T"]).T) * m
        env = P.gemm_envelope(a, op["w2T"], C) * m
        use["df"] = _located("df", 0, lambda: P.assert_within_rounding(got["df"], ref, env, 1, "df"))
        # db1 sums the masked fp32 accumulators in front of their rounding: each within its GEMM envelope of the fp64 value
        use["db1"] = _check_partial(parts, "db1", ref, env, "db1")
        del ref, env
        dh2 = f64(got["df"]) @ f64(op["w1T"]).T
        _check_ln_bwd(use, "2", got, parts, dh2, P.gemm_envelope(got["df"], op["w1T"], 4 * C), op["x1"], op["mean2"], op["rstd2"], op["ln2w"],
                      got["dx1"] if mode == 0 else op["dresid"], k2, True, max_share)
        ref = f64(got["g2"]) @ f64(op["wprojT"]).T
        use["dout"] = _located("dout", 0, lambda: P.assert_within_rounding(got["dout"], ref, P.gemm_envelope(got["g2"], op["wprojT"], C), 1, "dout"))
    return use


BWD_DEFECTS = ("dx1_row_without_residual", "dx2_row_without_mean_term", "g2_row_without_inv_keep", "dgamma2_wave_row_partial_dropped",
               "dbeta1_row_left_out", "df_chunk_unmasked", "dout_last_row_zero")
BWD_DEFECT_STAGE = dict(dx1_row_without_residual="dx1", dx2_row_without_mean_term="dx2", g2_row_without_inv_keep="g2",
                        dgamma2_wave_row_partial_dropped="dgamma2, partial rows", dbeta1_row_left_out="dbeta1, partial rows",
                        df_chunk_unmasked="df", dout_last_row_zero="dout")


def bwd_standin(op, mode, p, defect=None):
    """fp64 with a rounding at each of the kernel's rounding points: dh / dh2 to bf16 in front of the LayerNorm backward, x-hat to
    bf16 across the exchange, dx / g / df / dout as stored; partial sums in fp64 per (block, wave row), stored as fp32"""
    M = op["x"].shape[0]
    has_q, has_2 = mode in (0, 2), mode in (0, 1)
    k1, k2 = keep_scales(M, p, SITE_FFN, SITE_PROJ)
    out, parts = {}, torch.zeros(2 * (M // ROWS), PART_STRIDE)
    r0 = min(M - 1, ROWS + 33)

    def put(name, terms):
        a, w = PART_COLS[name]
        parts[:, a:a + w] = terms.view(M // 32, 32, w).sum(1).float()

    def half(tag, dh_exact, x, mean, rstd, gamma, dresid, scale, has_bias):
        dh = P.rb(dh_exact)
        o, xh, _ = _ln_bwd_fp64(dh, x, mean, rstd, gamma, dresid, xh_round=True)
        if defect == f"dx{tag}_row_without_residual":
            o[r0] -= f64(dresid)[r0]
        if defect == f"dx{tag}_row_without_mean_term":
            o[r0] += f64(rstd)[r0] * (dh[r0] * f64(gamma)).mean()
        g = o if scale is None else scale * o
        if defect == f"g{tag}_row_without_inv_keep":
            g = g.clone()
            g[r0] *= 1.0 - p
        out["dx" + tag], out["g" + tag] = o.float().to(bf), g.float().to(bf)
        put(f"dln{tag}w", dh * xh)
        if defect == f"dbeta{tag}_row_left_out":
            dh_b = dh.clone()
            dh_b[r0] = 0
            put(f"dln{tag}b", dh_b)
        else:
            put(f"dln{tag}b", dh)
        if has_bias:
            put("gbias" + tag, g)
        if defect == f"dgamma{tag}_wave_row_partial_dropped":
            a, w = PART_COLS[f"dln{tag}w"]
            parts[2 * (r0 // ROWS) + 1, a:a + w] = 0
    if has_q:
        half("1", f64(op["dqkv"]) @ f64(op["wqkvT"]).T, op["x"], op["mean1"], op["rstd1"], op["ln1w"], op["dresid"], k1 if mode == 0 else None, mode == 0)
    if has_2:
        a = out["g1"] if mode == 0 else op["g_in"]
        v = (f64(a) @ f64(op["w2T"]).T).float()
        m = op["mask"].clone()
        if defect == "df_chunk_unmasked":
            m[r0, 2 * C + 96:2 * C + 104] = 1
        v = v * m
        out["df"] = v.to(bf)
        put("db1", f64(v))
        half("2", f64(out["df"]) @ f64(op["w1T"]).T, op["x1"], op["mean2"], op["rstd2"], op["ln2w"], out["dx1"] if mode == 0 else op["dresid"], k2, True)
        out["dout"] = (f64(out["g2"]) @ f64(op["wprojT"]).T).float().to(bf)
        if defect == "dout_last_row_zero":
            out["dout"][M - 1] = 0
    return out, parts
