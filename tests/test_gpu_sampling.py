"""GPU: dg_sample_rows against its fp64 restatement (tests/sampling_model.py), and the two device-position decode kernels
(dg_embed_window, dg_attn_decode_append) against their host-position counterparts, bit for bit.

Tolerance d of the CDF test.  The kernel takes z_j - max in fp32 exactly as the restatement does, and from there on works in
fp64 (csrc/sample.hip): e_j = exp(.) to 1 ulp = 2^-53 relative, chunk sums of at most 52 terms in index order, a 6-level
shuffle scan and at most 16 wave totals, i.e. a summation depth of ~74: each prefix sum and S are within ~(74 + 1) * 2^-53 =
8e-15 relative of exact, and so is C(n) / S against F[n].  d = 2^-40 = 9e-13 leaves two orders of magnitude for the restatement's
own cumsum over 50257 terms (<= 50257 * 2^-53 = 6e-12 worst case, ~1e-14 typical) -- far below the 1e-5 cap.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

D_TOL = 2.0 ** -40
assert D_TOL <= 1e-5


def randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _near(F_row, u):
    """is u within D_TOL of a boundary of the CDF F_row?"""
    i = np.searchsorted(F_row, u)
    d = np.minimum(np.abs(F_row[np.minimum(i, F_row.size - 1)] - u), np.abs(F_row[np.maximum(i - 1, 0)] - u))
    return d < D_TOL


def check_against_restatement(dev, x_cpu, seed, L, temperature=1.0, top_k=None, ldl=None, pad=None):
    """x_cpu fp32 [M, V].  Runs the kernel (tokens + probs) and checks both against the fp64 restatement."""
    from drakegpt_amd import ops
    M, V = x_cpu.shape
    if ldl is None:
        xd = x_cpu.to(dev)
    else:
        buf = torch.empty((M, ldl), dtype=torch.float32)
        buf[:, V:] = pad
        buf[:, :V] = x_cpu
        xd = buf.to(dev)[:, :V]
    toks, p_gpu = ops.sample_rows(xd, seed=seed, L=L, temperature=temperature, top_k=top_k, probs=True)
    toks, p_gpu = toks.cpu().numpy(), p_gpu.cpu().numpy().astype(np.float64)
    e, kept = SM.weights(x_cpu.numpy(), temperature, top_k)
    S = e.sum(axis=1, keepdims=True)
    p = e / S
    # probs: one rounding to fp32 away from fp64; exactly 0 off the kept set; same kept set
    assert ((p_gpu > 0) == kept).all()
    err = np.abs(p_gpu - p)
    print(f"probs: max err / p = {np.max(err[kept] / p[kept]) / 2.0 ** -24:.2f} x 2^-24")
    assert (err <= 4 * 2.0 ** -24 * p + 1e-30).all()
    # tokens: F[n - 1] - d <= u < F[n] + d on the kept set
    F = np.cumsum(e, axis=1) / S
    u = SM.uniforms(seed, L, M)
    assert ((0 <= toks) & (toks < V)).all()
    rows = np.arange(M)
    assert kept[rows, toks].all()
    hi = F[rows, toks]
    lo = np.where(toks > 0, F[rows, np.maximum(toks - 1, 0)], 0.0)
    assert (lo - D_TOL <= u).all() and (u < hi + D_TOL).all()
    # the tolerance must not be able to hide an off-by-one: few u are that close to a boundary at all (a CPU-side statement about
    # the case; with few rows it is taken over 4096 uniforms per row)
    near = (np.abs(F - u[:, None]) < D_TOL).any(axis=1) if V <= 8192 else np.array([_near(F[m], u[m:m + 1])[0] for m in range(M)])
    share = near.mean() if M >= 1024 else np.mean([_near(F[m], SM.uniforms(seed, L, 4096)).mean() for m in range(M)])
    print(f"u within d of a boundary: {share:.4%}")
    assert share < 0.01
    # and away from the boundaries the tokens are the restatement's, exactly
    ref = np.array([SM._pick(e[m], kept[m], u[m:m + 1])[0] for m in range(M)])
    assert (toks[~near] == ref[~near]).all()
    return toks, p_gpu, kept


@pytest.mark.parametrize("V,M,ldl,top_k,temperature", [
    (80, 8192, None, None, 1.0),          # many workgroups
    (257, 3, 264, None, 1.0),             # ragged row, padding columns that must never be read
    (50257, 4, None, None, 1.0),          # the 1024-thread kernel, 50 elements per thread (logits x 8, as in the host table)
    (50257, 4, None, 50, 1.0),            # radix select over a long row
    (8192, 2, None, 40, 0.7),             # the last size of the 256-thread kernel (32 elements per thread)
    (8193, 2, None, 40, 1.3),             # the first size of the 1024-thread kernel
    (80, 1, None, None, 1.0),
    (80, 64, None, 10, 0.7),
])
def test_kernel_matches_restatement(dev, V, M, ldl, top_k, temperature):
    x = randn((M, V), 3 + V, scale=8.0 if (V == 50257 and top_k is None) else 1.0)
    pad = None
    if ldl is not None:
        pad = torch.tensor([float("nan"), float("inf")] * ((ldl - V + 1) // 2))[:ldl - V]
    check_against_restatement(dev, x, 1234, 5, temperature, top_k, ldl, pad)


def test_top_k_edges(dev):
    from drakegpt_amd import ops
    V, M = 300, 16
    x = randn((M, V), 9)
    xd = x.to(dev)
    # top_k = 1 is the argmax whatever u is
    t1 = ops.sample_rows(xd, seed=7, L=3, top_k=1)
    assert torch.equal(t1.cpu(), x.argmax(1))
    # top_k = V is "off": same tokens, same probs, bit for bit
    tV, pV = ops.sample_rows(xd, seed=7, L=3, top_k=V, probs=True)
    t0, p0 = ops.sample_rows(xd, seed=7, L=3, probs=True)
    assert torch.equal(tV, t0) and torch.equal(pV, p0)
    # ties that straddle the threshold: the 5 largest are {4, 3, 3, 3, 3, 3}-ish -> top_k = 3 keeps all the 3s
    y = randn((M, V), 10).clamp(max=2.0)
    y[:, 17] = 4.0
    for c in (5, 100, 101, 250, 299):
        y[:, c] = 3.0
    _, p, kept = check_against_restatement(dev, y, 7, 4, 1.0, 3)
    assert (kept.sum(1) == 6).all()
    assert (p[:, [5, 100, 101, 250, 299]] > 0).all()


def test_special_rows(dev):
    from drakegpt_amd import ops
    V, M = 1000, 8
    x = randn((M, V), 21)
    # greedy: torch.argmax, and the LOWEST index on planted ties
    x[1, 700] = x[1, 30] = x[1, 31] = 9.0
    x[2, V - 1] = x[2, 0] = 9.0
    xd = x.to(dev)
    tg, pg = ops.sample_rows(xd, seed=1, L=0, temperature=0.0, probs=True)
    want = x.argmax(1)
    want[1], want[2] = 30, 0
    assert torch.equal(tg.cpu(), want)
    assert torch.equal(pg.cpu(), torch.nn.functional.one_hot(want, V).float())
    # greedy consumes no random number: any state gives the same token
    assert torch.equal(ops.sample_rows(xd, seed=99, L=123, temperature=0.0), tg)
    # an all-equal row: uniform probs
    eq = torch.full((2, V), -1.25)
    te, pe = ops.sample_rows(eq.to(dev), seed=5, L=2, probs=True)
    assert torch.equal(pe.cpu(), torch.full((2, V), np.float32(1.0 / V)))
    assert te.cpu().tolist() == np.floor(SM.uniforms(5, 2, 2) * V).astype(int).tolist()       # e_j = 1: every sum is exact
    # -inf entries are never returned, whatever u is: all rows share the logits, 4096 different u
    z = randn((V,), 22)
    z[::2] = float("-inf")
    z[V - 1] = float("-inf")
    rows = z.repeat(4096, 1)
    tz, pz = ops.sample_rows(rows.to(dev), seed=8, L=77, probs=True)
    assert torch.isfinite(z[tz.cpu()]).all()
    assert (pz.cpu()[:, ::2] == 0).all()
    check_against_restatement(dev, rows[:64].contiguous(), 8, 77)
    # tokens written in place: ids[m, L], nothing else touched; L beyond the buffer writes nothing
    ids = torch.full((M, 12), -7, dtype=torch.int64, device=dev)
    st = ops.new_rng_state(1234, dev, step=9)
    ops.sample_rows(xd, st, ids=ids)
    direct = ops.sample_rows(xd, seed=1234, L=9)
    assert torch.equal(ids[:, 9], direct)
    ids[:, 9] = -7
    assert (ids == -7).all()
    ops.sample_rows(xd, ops.new_rng_state(1234, dev, step=12), ids=ids)
    torch.cuda.synchronize()
    assert (ids == -7).all()


@pytest.mark.parametrize("seed,L,top_k,temperature", [(1234, 5, None, 1.0), (1234, 6, 10, 0.7), (7, 300, None, 1.0)])
def test_kernel_frequencies(dev, seed, L, top_k, temperature):
    """8192 rows of identical logits: the kernel's token frequencies obey the 5-sigma binomial bound of test_sampling_host"""
    from drakegpt_amd import ops
    x = randn((80,), 3)
    toks = ops.sample_rows(x.repeat(8192, 1).to(dev), seed=seed, L=L, top_k=top_k, temperature=temperature).cpu().numpy()
    p, kept = SM.probs(x.numpy(), temperature, top_k)
    ok, worst = SM.freq_bound_ok(toks, p)
    print(f"worst standardised deviation {worst:.2f} sigma")
    assert ok, worst


# --------------------------------------------------------------------------------------------------------------------------
GUARD = 256


def guarded(shape, dtype, dev, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[-GUARD:] == fill).all())


def test_embed_window_equals_embed_fwd(dev):
    from drakegpt_amd import ops
    B, Tw, C, V, cap = 2, 65, 48, 80, 80
    g = torch.Generator().manual_seed(4)
    ids = torch.randint(0, V, (B, cap), generator=g).to(dev)
    ids[0, 3], ids[1, 70] = V + 5, -2                              # clamped like dg_embed_fwd clamps
    tok, pos = randn((V, C), 5).to(dev), randn((Tw, C), 6).to(dev)
    for t in (0, 1, 63, 64):                                       # mode 0 at position t = L - 1
        st = ops.new_rng_state(0, dev, step=t + 1)
        buf, out = guarded((B, C), torch.float32, dev, 777.0)
        ops.embed_window(ids, st, tok, pos, 0, out=out)
        ref = ops.embed_fwd(ids[:, t:t + 1].contiguous(), tok, pos[t:t + 1])
        assert torch.equal(out, ref.view(B, C)) and guards_intact(buf, 777.0)
    for L in (65, 66, 80):                                         # mode 1: the last Tw ids
        st = ops.new_rng_state(0, dev, step=L)
        buf, out = guarded((B, Tw, C), torch.float32, dev, 777.0)
        ops.embed_window(ids, st, tok, pos, 1, out=out)
        ref = ops.embed_fwd(ids[:, L - Tw:L].contiguous(), tok, pos)
        assert torch.equal(out, ref) and guards_intact(buf, 777.0)
    for mode, L in ((0, 0), (0, 66), (1, 64), (1, 81), (0, 2 ** 31 + 5)):      # outside the mode's range / the ids: nothing is written
        st = ops.new_rng_state(0, dev, step=L)
        buf, out = guarded((B, C) if mode == 0 else (B, Tw, C), torch.float32, dev, 777.0)
        ops.embed_window(ids, st, tok, pos, mode, out=out)
        torch.cuda.synchronize()
        assert (buf == 777.0).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_attn_decode_append_equals_attn_decode(dev, dtype):
    from drakegpt_amd import ops
    B, NH, H, Tcap = 2, 4, 16, 65
    W = 3 * NH * H
    cache0 = randn((B, Tcap, W), 7).to(dtype)
    for t in (0, 1, 63, 64):
        row = randn((B, W), 100 + t).to(dtype).to(dev)
        cbuf, cache = guarded((B, Tcap, W), dtype, dev, 55.0)
        cache.copy_(cache0)
        obuf, out = guarded((B, NH * H), dtype, dev, 55.0)
        ref_cache = cache0.to(dev).clone()
        ref_cache[:, t] = row
        ref = ops.attn_decode(ref_cache, t, NH, H, H ** -0.5)
        ops.attn_decode_append(row, cache, ops.new_rng_state(0, dev, step=t + 1), NH, H, H ** -0.5, out=out)
        assert torch.equal(out, ref), t
        assert torch.equal(cache, ref_cache), t
        assert guards_intact(cbuf, 55.0) and guards_intact(obuf, 55.0)
    for L in (0, Tcap + 1, 2 ** 31 + 1):                           # t = L - 1 outside the cache: nothing is written
        row = randn((B, W), 1).to(dtype).to(dev)
        cbuf, cache = guarded((B, Tcap, W), dtype, dev, 55.0)
        obuf, out = guarded((B, NH * H), dtype, dev, 55.0)
        ops.attn_decode_append(row, cache, ops.new_rng_state(0, dev, step=L), NH, H, H ** -0.5, out=out)
        torch.cuda.synchronize()
        assert (cbuf == 55.0).all() and (obuf == 55.0).all()
