"""Structured operands: the inputs on which a kernel's numerics are decided, each against fp64 on the same operands.

Everything else in the suite feeds iid randn.  Here: attention scores whose running maximum moves at every key tile (up and
down), near one-hot and uniform softmax rows, rows whose every kept probability was dropped, identical keys; LayerNorm rows
with a mean far above their spread, tiny rows, constant rows, an outlier; cross-entropy rows with logit ranges of 30 .. 2000 and
the target at either end; AdamW with zero, tiny and huge gradients.  Bounds are derived beside each check (oracle/parity.py for
the shared ones); none is taken from a kernel's output."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
bf = torch.bfloat16


def _ops():
    from drakegpt_amd import ops
    return ops


def _report(msg):
    if os.environ.get("DG_TEST_REPORT"):
        print("[conditioning] " + msg, flush=True)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _attn_operands(kind, B, T, NH, H, g):
    """q, k, v [B, T, NH, H] fp32"""
    rn = lambda *s: torch.randn(*s, generator=g)
    q, k, v = rn(B, T, NH, H), rn(B, T, NH, H), rn(B, T, NH, H)
    u = torch.ones(H) / H ** 0.5                                   # |u| = 1
    a = (3.0 * H ** 0.5) ** 0.5                                    # (a u) . (a u) * H^-1/2 = 3
    tile = (torch.arange(T) // 32).float().view(1, T, 1, 1)
    if kind == "rising":                                           # q . k_j * scale ~ +3 per 32-key tile
        q, k = a * u + 0.1 * q, a * u * tile + 0.1 * k
    elif kind == "falling":
        q, k = a * u + 0.1 * q, a * u * (tile.max() - tile) + 0.1 * k
    elif kind == "onehot":                                         # scores ~ N(0, 60^2): q . k = 60 sum z z', times H^-1/2
        q, k = q * 60 ** 0.5, k * 60 ** 0.5
    elif kind == "uniform":                                        # all scores equal
        q = torch.zeros_like(q)
    elif kind == "same_keys":                                      # identical keys, distinct values
        k = k[:, :1].expand(B, T, NH, H).contiguous()
    elif kind != "randn":
        raise ValueError(kind)
    return q, k, v


ATTN_KINDS = [("rising", 256, 0.0), ("rising", 1024, 0.1), ("falling", 256, 0.1), ("falling", 1024, 0.0), ("onehot", 256, 0.0), ("uniform", 256, 0.1),
              ("same_keys", 256, 0.0), ("randn", 8, 0.9), ("randn", 64, 0.9)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32-generic", "bf16-mfma"])
@pytest.mark.parametrize("kind,T,p", ATTN_KINDS)
def test_attention_structured_scores(dev, dtype, kind, T, p):
    from oracle import parity as P
    from oracle import rng_ref
    ops = _ops()
    B, NH, H = (4, 4, 64) if T <= 64 else (1, 2, 64)
    C = NH * H
    g = torch.Generator().manual_seed(T + len(kind))
    q, k, v = _attn_operands(kind, B, T, NH, H, g)
    qkv = torch.stack([q, k, v], 2).reshape(B * T, 3 * C).to(dtype)
    dout = torch.randn(B * T, C, generator=g).to(dtype)
    lowp = dtype == bf
    assert ops.attn_fp8_out_supported(B, T, NH, H, dtype) == lowp          # which family runs: MFMA for bf16 at H = 64, even T
    seed, step, site = 5, 2, 8
    keep = rng = None
    if p > 0:
        keep = torch.from_numpy(rng_ref.keep_mask(seed, step, site, p, B * NH * T * T).reshape(B, NH, T, T)).double()
        rng = ops.new_rng_state(seed, dev, step)
    R = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p)
    Mo = P.attention_fp64(qkv, dout, B, T, NH, H, keep, p, model=True if lowp else "fp32")
    out, lse = ops.attn_fwd(qkv.to(dev), B, T, NH, H, H ** -0.5, p, rng, site, keep=True)
    dqkv = ops.attn_bwd(qkv.to(dev), out, dout.to(dev), lse, B, T, NH, H, H ** -0.5, p, rng, site)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
    # forward, element-wise.  bf16: oracle/parity.py's envelope 2^-8 (Pd |V|) + one output rounding.  Both families compute a score as an
    # fp32 sum of H exact products: |s - s_exact| <= H 2^-24 sum_d |q_d k_d| scale =: ds, and a probability moves by the factor
    # exp(+-2 ds) (its own score and the row's normaliser) -- invisible at |s| ~ 3, not at |s| ~ 60.  fp32 adds one rounding per
    # probability and per term of the length-(<= T) P V sum: (T + 2) 2^-24 (Pd |V|).
    qd, kd, _ = (t.to(dtype).double().permute(0, 2, 1, 3) for t in (q, k, v))
    ds = H * 2.0 ** -24 * (qd.abs() @ kd.abs().transpose(-2, -1)).amax(-1) * H ** -0.5                       # [B, NH, T], worst key of the row
    pv = P.attention_fwd_envelope(R) / P.BF16_RN                                                            # Pd |V|, packed like out
    spread = torch.expm1(2 * ds).permute(0, 2, 1).reshape(B * T, NH).repeat_interleave(H, 1) * pv
    if lowp:
        use = P.assert_within_rounding(out, R["out"], P.BF16_RN * pv + spread, 1, f"{kind} forward")
    else:
        use = P.assert_within_rounding(out, R["out"], (T + 2) * 2.0 ** -24 * pv + spread + 2.0 ** -23 * R["out"].abs(), 0, f"{kind} forward")
    # lse is fp32 arithmetic on exact products for fp32 and bf16 operands alike
    el = ((lse.double().cpu() - R["lse"]).abs() / R["lse"].abs().clamp_min(1)).max().item()
    assert el < 1e-5, el
    if keep is not None:
        # rows whose every kept probability was dropped: exactly zero
        dead = (keep * torch.tril(torch.ones(T, T, dtype=torch.float64))).sum(-1) == 0                       # [B, NH, T]
        assert p < 0.5 or int(dead.sum()) > 0
        o4 = out.float().cpu().view(B, T, NH, H).permute(0, 2, 1, 3)
        assert torch.all(o4[dead] == 0)
    # backward: per (row, head) and gradient third within BWD_MARGIN x the rounding model's worst group around the same position, and
    # never below the suite's fp32 tolerance (both families accumulate in fp32; on these operands the model's error is exactly
    # zero in whole groups).  Denominators floored by oracle/parity.py's structured_floor: these gradients are heavy-tailed or cancel.
    floors = {n: P.structured_floor(R, n, H) for n in ("dq", "dk", "dv")}
    bounds = P.attention_bwd_bounds_by_position(R, Mo, B, T, NH, H, at_least=3e-5, floors=floors)
    uses = {}
    for i, n in enumerate(("dq", "dk", "dv")):
        # the bound means something.  dk, dv: a zeroed group fails it.  dq on these operands is a cancellation in most rows (the
        # keys share a direction, or the row is one-hot), the model's own error there is of order 0.1 .. 0.5 of the floor, and the
        # bound of order 1: it catches a wrong scale or sign and anything non-finite, not a single damaged group
        assert bounds[n].max().item() < 10 and (n == "dq" or bounds[n].median().item() < 0.1), (n, bounds[n].median().item(), bounds[n].max().item())
        uses[n] = P.assert_rowwise_each(dqkv.view(B * T, 3, C)[:, i], R[n], H, bounds[n], f"{kind} T={T} {n}", T, floor=floors[n])
    _report(f"attention {kind} T={T} p={p} {'bf16' if lowp else 'fp32'}: forward envelope use {use:.2f}, lse {el:.1e}, backward use "
            + " ".join(f"{n} {u:.2f}" for n, u in uses.items()))


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def _ln_rows(kind, M, C, g):
    x = torch.randn(M, C, generator=g)
    if kind == "offset":
        return 1000.0 + x
    if kind == "tiny":
        return 1e-3 * x
    if kind == "constant":                                        # C * c is exact in fp32 for these: the row mean is c itself
        return torch.tensor([0.0, 4.0, -2.5, 1024.0])[torch.arange(M) % 4].view(M, 1).expand(M, C).contiguous()
    if kind == "outlier":
        x[torch.arange(M), torch.arange(M) % C] = 1e4
        return x
    raise ValueError(kind)


# the fp64 LayerNorm and the envelope of its fp32 evaluation: shared with tests/test_gpu_chain_parity.py
from oracle.parity import layernorm_envelope as _ln_envelope, layernorm_fp64 as _ln_fp64  # noqa: E402


@pytest.mark.parametrize("C", [384, 1024, 100])
@pytest.mark.parametrize("kind", ["offset", "tiny", "constant", "outlier"])
def test_layernorm_conditioning(dev, kind, C):
    from oracle import parity as P
    ops = _ops()
    M, G = 130, 8
    g = torch.Generator().manual_seed(C + len(kind))
    x = _ln_rows(kind, M, C, g)
    w, b = 1 + 0.1 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    dy = torch.randn(M, C, generator=g)
    ref, mean, std, xhat = _ln_fp64(x, w, b)
    env = _ln_envelope(mean, std, xhat, w)
    y, mu, rstd = ops.layernorm_fwd(x.to(dev), w.to(dev), b.to(dev), torch.float32)
    use = P.assert_within_rounding(y, ref, env + 2.0 ** -23 * ref.abs(), 0, f"layernorm {kind}")
    yb, _, _ = ops.layernorm_fwd(x.to(dev), w.to(dev), b.to(dev), bf)
    P.assert_within_rounding(yb, ref, env + 2.0 ** -23 * ref.abs(), 1, f"layernorm {kind}, bf16 out")
    if kind == "constant":
        assert torch.equal(y.cpu(), b.expand(M, C)) and torch.equal(yb.cpu(), b.bfloat16().expand(M, C))     # x - mean == 0: beta exactly
        assert torch.allclose(rstd.cpu(), torch.full((M,), 1e-5 ** -0.5), rtol=1e-6)
    # backward: dx = rstd (a - mean(a) - xhat mean(a xhat)), a = gamma dy.  With xhat off by e (the forward's bound without gamma):
    # |mean(a xhat)| <= max|a| (rms(xhat) <= 1) and its change <= e max|a|, so dx moves by <= rstd max|a| e (1 + max|xhat|); the two
    # length-C fp32 means add C 2^-23 of the same product; the result's own rounding is the |ref| term.
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    F.layer_norm(xd, (C,), wd, bd, 1e-5).backward(dy.double())
    amax = (w.double() * dy.double()).abs().amax(1, keepdim=True)
    e = env / w.double().abs()
    benv = (amax / std) * (1 + xhat.abs().amax(1, keepdim=True)) * (e.amax(1, keepdim=True) + C * 2.0 ** -23)
    pg, pb = torch.empty(G, C, device=dev), torch.empty(G, C, device=dev)
    dx = ops.layernorm_bwd(dy.to(dev), x.to(dev), w.to(dev), mu, rstd, None, pg, pb, C, G)
    assert torch.isfinite(dx).all() and torch.isfinite(pg).all() and torch.isfinite(pb).all()
    ub = P.assert_within_rounding(dx, xd.grad, benv + 2.0 ** -22 * xd.grad.abs(), 0, f"layernorm backward {kind}")
    if ops.layernorm_bwd_fused_supported(C):
        pq = torch.empty(G, C, device=dev)
        dx2, g2 = ops.layernorm_bwd_fused(dy.to(dev), x.to(dev), w.to(dev), mu, rstd, None, pg, pb, C, G, bf, 0.0, None, 0, pq)
        assert torch.isfinite(dx2).all() and torch.isfinite(g2.float()).all()
        P.assert_within_rounding(dx2, xd.grad, benv + 2.0 ** -22 * xd.grad.abs(), 0, f"fused layernorm backward {kind}")
        P.assert_within_rounding(g2, xd.grad, benv + 2.0 ** -22 * xd.grad.abs(), 1, f"fused layernorm backward {kind}, bf16 g")
    _report(f"layernorm {kind} C={C}: forward use {use:.2f}, backward use {ub:.2f}")


@pytest.mark.parametrize("mode", [3, 4])
def test_chain_layernorm_on_offset_rows(dev, mode):
    """dg_block_chain_fwd modes 3 / 4 (a row-complete GEMM with a LayerNorm in the epilogue, C = 384: four 96-column partial
    statistics combined by Chan's formula) on a residual stream of 1000 + randn, against fp64 on the launch's own fp32 GEMM
    output -- not only against the separate LayerNorm launch, which could share a defect"""
    from oracle import parity as P
    ops = _ops()
    M, C = 4160, 384
    g = torch.Generator().manual_seed(mode)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x = (1000.0 + rn(M, C)).to(dev)
    Vv = {k: v.to(dev) for k, v in dict(bproj=rn(C, sc=0.1), b1=rn(4 * C, sc=0.1), b2=rn(C, sc=0.1), ln2w=1 + rn(C, sc=0.1), ln2b=rn(C, sc=0.1),
                                        ln1w=1 + rn(C, sc=0.1), ln1b=rn(C, sc=0.1)).items()}
    W = {k: ops.pack_chain_weights(v.to(bf).to(dev)) for k, v in dict(wproj=rn(C, C, sc=C ** -0.5), w1=rn(4 * C, C, sc=C ** -0.5),
                                                                      w2=rn(C, 4 * C, sc=(4 * C) ** -0.5), wqkv=rn(3 * C, C, sc=C ** -0.5)).items()}
    if mode == 3:
        got = ops.block_chain_fwd(3, M, C, o=rn(M, C).to(bf).to(dev), x=x, **W, **Vv)
        pre, h, w, b, mu, rs = got["x1"], got["h2"], Vv["ln2w"], Vv["ln2b"], got["mean2"], got["rstd2"]
    else:
        got = ops.block_chain_fwd(4, M, C, f=rn(M, 4 * C).clamp_min(0).to(bf).to(dev), x1=x, **W, **Vv)
        pre, h, w, b, mu, rs = got["x2"], got["h1"], Vv["ln1w"], Vv["ln1b"], got["mean1"], got["rstd1"]
    torch.cuda.synchronize()
    ref, mean, std, xhat = _ln_fp64(pre.cpu(), w.cpu(), b.cpu())
    assert (mean.abs() / std).min().item() > 500                                     # the rows ARE badly conditioned
    env = _ln_envelope(mean, std, xhat, w.cpu())
    use = P.assert_within_rounding(h, ref, env + 2.0 ** -23 * ref.abs(), 1, f"chain mode {mode} LayerNorm")
    # the statistics themselves: the mean within 4 fp32 roundings of its size; rstd inherits (mean error / std) relative
    assert ((mu.double().cpu() - mean.view(-1)).abs() <= 4 * 2.0 ** -24 * mean.abs().view(-1)).all()
    assert ((rs.double().cpu() * std.view(-1) - 1).abs() <= 4 * 2.0 ** -24 * (mean.abs() / std + 1).view(-1) * xhat.abs().amax(1) + 2.0 ** -22).all()
    _report(f"chain mode {mode} LayerNorm on offset rows: envelope use {use:.2f}")


# ---------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------
def _ce_rows(M, V, rng_, g):
    """bf16-representable logits in [0, rng_] (row maximum rng_ itself), rows 0 .. 4 special; returns logits, targets (raw), targets (clamped)"""
    x = (torch.rand(M, V, generator=g) * rng_).bfloat16().float()
    x[:, 0] = float(torch.tensor(float(rng_)).bfloat16())
    x[:, 1] = 0.0
    perm = torch.stack([torch.randperm(V, generator=g) for _ in range(M)])
    x = torch.gather(x, 1, perm)
    tgt = torch.randint(0, V, (M,), generator=g)
    top = x[0].argmax()
    x[0] = (x[0] / 3).bfloat16().float()                          # the others at least 2/3 of the range below the maximum: loss ~ 0
    x[0, top] = x[1].max()
    tgt[0] = top
    tgt[1] = x[1].argmin()                                        # loss ~ range
    x[2] = x[2, 0]                                                # all equal: loss = ln V
    raw = tgt.clone()
    raw[3], raw[4] = -1, V                                        # clamped to 0 and V - 1, as the kernels document
    tgt[3], tgt[4] = 0, V - 1
    return x, raw, tgt


# kernel, logits dtype, V, leading dimension
CE_KERNELS = [("small", torch.float32, 80, 80), ("generic", torch.float32, 1000, 1000), ("row-fp32", torch.float32, 5000, 5000),
              ("row-bf16-vec", bf, 5000, 5000), ("row-bf16-unaligned", bf, 5001, 5001), ("fused-head", torch.float32, 80, 88)]


@pytest.mark.parametrize("rng_", [30, 200, 2000])
@pytest.mark.parametrize("kernel,ldt,V,ld", CE_KERNELS, ids=[c[0] for c in CE_KERNELS])
def test_cross_entropy_logit_ranges(dev, kernel, ldt, V, ld, rng_):
    from oracle import parity as P
    ops = _ops()
    M = 64
    g = torch.Generator().manual_seed(V + rng_)
    x, raw, tgt = _ce_rows(M, V, rng_, g)
    xd = x.double()
    mx = xd.amax(1)
    ref = torch.logsumexp(xd, 1) - xd[torch.arange(M), tgt]
    assert ref[0] < 1e-4 and ref[1] > 0.9 * rng_ and abs(ref[2].item() - math.log(V)) < 1e-9
    ref_grad = (torch.softmax(xd, 1) - F.one_hot(tgt, V)) / M
    buf = torch.zeros(M, ld, dtype=ldt)
    buf[:, :V] = x.to(ldt)
    logits = buf.to(dev)[:, :V]
    for gdt in ((bf,) if ldt == bf else (torch.float32, bf)):
        dl = torch.full((M, ld), float("nan"), dtype=gdt, device=dev)
        if kernel == "fused-head":
            n = 7
            scratch, loss = torch.zeros(n + 1, device=dev), torch.zeros((), device=dev)
            rows = ops.cross_entropy_fused(logits, raw.to(dev), V, dl, 1.0 / M, None, 0, n, scratch, loss, 1.0 / M)
            assert abs(loss.item() - ref.mean().item()) <= 2.0 ** -22 * (mx.mean().item() + ref.mean().item()) + M * 2.0 ** -24 * ref.mean().item()
        else:
            rows = ops.cross_entropy(logits, raw.to(dev), V, dlogits=dl, grad_scale=1.0 / M)
        torch.cuda.synchronize()
        err = (rows.double().cpu() - ref).abs()
        if kernel == "row-bf16-vec":
            # exp2(fma(x, log2e, -fl(mx log2e))): the rounding of mx log2e (2^-24 |mx| log2e) is a common factor 2^eps of every term,
            # i.e. eps ln2 on the loss; the sum mx + log(s) - x_t is fp32 arithmetic on numbers of size |mx| and |loss|
            bound = 2.0 ** -24 * mx.abs() * 1.4426950408889634 * 0.6931471805599453 + 2.0 ** -22 * ref.abs()
        else:
            # exp(x - mx) with x - mx exact; mx + log(s) - x_t: two fp32 additions on numbers of size |mx| and |loss|
            bound = 2.0 ** -22 * mx.abs() + 2.0 ** -22 * ref.abs()
        assert bool((err <= bound).all()), (kernel, rng_, int((err > bound).sum()), (err / bound).max().item(), int((err / bound).argmax()))
        assert torch.isfinite(dl[:, :V].float()).all() and torch.all(dl[:, V:] == 0)
        P.assert_within_rounding(dl[:, :V], ref_grad, P.single_rounding_envelope(ref_grad, V), 1 if gdt == bf else 0, f"{kernel} gradient, range {rng_}")
        _report(f"cross entropy {kernel} range {rng_} grad {gdt}: loss use {(err / bound).max().item():.2f}")


# ---------------------------------------------------------------------------------------------------------------------
# AdamW
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zero", "tiny", "huge", "mixed"])
def test_adamw_extreme_gradients(dev, kind):
    """zero / denormal second moments (g = 0; g = 1e-30, whose square underflows in fp32) and g = 1e15 (g^2 = 1e30 still
    finite), three steps against the oracle's AdamW evaluated in fp64.  |p - ref| <= 2e-6 max(1, |ref|): the level of
    test_adamw_matches_oracle, relative where a weight has grown (an update cannot be resolved below an fp32 ulp of the weight
    it is added to, so the comparison is on the weight); nothing non-finite; the bf16 shadow is the rounding of the weights."""
    from oracle import drake_ref as R
    ops = _ops()
    n = 10007
    g = torch.Generator().manual_seed(len(kind))
    p0 = torch.randn(n, generator=g)
    params = {"w": p0.double().clone()}
    opt = R.AdamWState(["w"], 1e-3, (0.9, 0.95))
    pd = p0.clone().to(dev)
    pad = (n + 3) // 4 * 4
    m, v = torch.zeros(pad, device=dev)[:n], torch.zeros(pad, device=dev)[:n]
    hyper = torch.tensor([1e-3, 0.9, 0.95, 1e-8, 1e-2], device=dev)
    st = ops.new_rng_state(0, dev, 0)
    shadow = torch.empty(n, dtype=bf, device=dev)
    levels = dict(zero=[0.0], tiny=[1e-30], huge=[1e15], mixed=[0.0, 1e-30, 1e15, 1.0, 1e-12])[kind]
    for it in range(3):
        sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        gr = sign * torch.tensor(levels)[torch.randint(0, len(levels), (n,), generator=g)]
        opt.step(params, {"w": gr.double()})
        ops.adamw_step(pd, gr.to(dev), m, v, hyper, st, shadow_bf16=shadow, advance=True)
    torch.cuda.synchronize()
    assert torch.isfinite(pd).all() and torch.isfinite(m).all() and torch.isfinite(v).all() and torch.isfinite(shadow.float()).all()
    ref = params["w"]
    err = (pd.double().cpu() - ref).abs()
    assert bool((err <= 2e-6 * ref.abs().clamp_min(1)).all()), (err / ref.abs().clamp_min(1)).max().item()
    assert torch.equal(shadow.cpu(), pd.cpu().bfloat16())
