"""GPU: dg_sample_rows_nucleus (top-p and min-p inside the sampler kernel) against its restatement (tests/nucleus_model.py), and
generate(top_p=, min_p=) end to end: graph-replayed, eager, host sampler, one of the smaller models.

What is demanded: the kept set (probs > 0) EXACTLY the restatement's, probs within 1e-6 relative, tokens equal.  The kept set
is decided by comparisons of doubles (G < T, e >= min_p); the device's fp64 exp may differ from numpy's in the last bit, which
moves G / S1 by at most ~V * 2^-53 = 6e-12 and e / min_p by 1e-16.  So every comparison first asserts, on the restatement alone,
that each row is at least 1e-8 away from such a decision (worst over the case table: 4.5e-6 for top-p, 5.1e-4 for min-p); no
row is excluded.  The token needs u * S clear of a CDF step by the same 1e-14: u has 24 bits, the chance per row is ~1e-7.
probs: e / S in fp64, one rounding to fp32 (2^-24 = 6e-8) -- 1e-6 holds with a decade to spare.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucleus_model as NM  # noqa: E402
import sampling_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu


def assert_clear(x, temperature=1.0, top_k=None, top_p=None, min_p=None):
    """the precondition of an exact comparison, stated on the restatement alone"""
    mg, mm = NM.margins(x, temperature, top_k, top_p, min_p)
    print(f"margins: top-p {mg.min():.2e}, min-p {mm.min():.2e}")
    assert (mg >= NM.MARGIN).all(), mg.min()
    assert (mm >= NM.MARGIN).all(), mm.min()


def check_against_restatement(dev, x, seed, L, temperature=1.0, top_k=None, top_p=None, min_p=None):
    """x fp32 numpy [M, V], handed to the kernel inside a wider buffer (ldl > V) whose padding must never be read"""
    from drakegpt_amd import ops
    assert_clear(x, temperature, top_k, top_p, min_p)
    M, V = x.shape
    buf = torch.empty((M, V + 7), dtype=torch.float32)
    buf[:, V:] = torch.tensor([float("nan"), float("inf"), 1e30, float("nan"), float("inf"), 1e30, float("nan")])
    buf[:, :V] = torch.from_numpy(x)
    xd = buf.to(dev)[:, :V]
    toks, p_gpu = ops.sample_rows(xd, seed=seed, L=L, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, probs=True)
    toks, p_gpu = toks.cpu().numpy(), p_gpu.cpu().numpy().astype(np.float64)
    p, kept = NM.probs(x, temperature, top_k, top_p, min_p)
    print(f"kept per row: {kept.sum(1).min()} .. {kept.sum(1).max()} of {V}")
    assert ((p_gpu > 0) == kept).all()
    rel = np.abs(p_gpu - p)[kept] / p[kept]
    print(f"probs: max relative error {rel.max():.2e}")
    assert rel.max() <= 1e-6
    ref = NM.sample(x, seed, L, temperature, top_k, top_p, min_p)
    assert (toks == ref).all(), np.flatnonzero(toks != ref)
    return toks, p_gpu, kept


@pytest.mark.parametrize("i", range(len(NM.CASES)))
def test_kernel_matches_restatement(dev, i):
    V, M, temperature, top_k, top_p, min_p = NM.CASES[i]
    x = NM.case_logits(i)
    assert x.shape == (M, V)
    _, _, kept = check_against_restatement(dev, x, 1234, 5 + i, temperature, top_k, top_p, min_p)
    assert (kept.sum(1) < V).all()                     # the filter did something in every row


@pytest.mark.parametrize("name", list(NM.hand_rows()))
def test_hand_made_rows(dev, name):
    x, kw, want = NM.hand_rows()[name]
    rows = np.repeat(x[None], 64, axis=0)              # 64 different u on the one row
    toks, _, kept = check_against_restatement(dev, rows, 3, 9, **kw)
    if want is None:
        assert kept.all()
    elif want == "finite":
        assert not kept[:, ~np.isfinite(x)].any() and np.isfinite(x[toks]).all()
    else:
        assert np.flatnonzero(kept[0]).tolist() == want


def test_masses_that_round_to_zero(dev):
    """{0, -100, ...}: every mass but the maximum's is rint(e^-100 * 2^40) = 0, so S1 is the maximum's alone and the rest has
    G = S1 >= T for every top_p < 1 -- also for the largest fp32 below 1"""
    V = 1000
    x = np.full((8, V), -100.0, dtype=np.float32)
    x[:, 421] = 0.0
    for top_p in (0.9, float(np.nextafter(np.float32(1), np.float32(0)))):
        toks, _, kept = check_against_restatement(dev, x, 2, 6, top_p=top_p)
        assert (kept.sum(1) == 1).all() and (toks == 421).all()
    # a tail that runs from below 2^-41 (no mass) up to e^-5: the kept set ends inside the part that has mass
    y = np.linspace(-40, -5, V).astype(np.float32)[None].repeat(8, axis=0)
    y[:, 7] = 0.0
    _, _, kept = check_against_restatement(dev, y, 2, 7, top_p=0.999)
    assert (kept.sum(1) > 1).all() and kept[:, 7].all() and not kept[:, 8:400].any()


@pytest.mark.parametrize("V", [1000, 9000])
def test_ties_across_chunk_edges(dev, V):
    """thread t of the blocked scan owns [t * chunk, (t + 1) * chunk): 4 elements of 256 threads at V = 1000, 9 of 1024 at
    V = 9000.  A tie group placed on both sides of thread, wave and last-chunk edges sits exactly at the top-p threshold: all of it
    is kept, nothing below it is."""
    NT = 256 if V <= 8192 else 1024
    chunk = (V + NT - 1) // NT
    x = np.random.default_rng(V).uniform(-12.0, -10.0, size=V).astype(np.float32)
    tie = [chunk - 1, chunk, 64 * chunk - 1, 64 * chunk, (V // chunk) * chunk - 1, min((V // chunk) * chunk, V - 1), V - 1]
    tie = sorted(set(tie))
    x[5] = 3.0                                          # one token above the tie group, ~0.27 of the mass
    x[tie] = 2.0                                        # the group: ~0.1 each
    rows = np.repeat(x[None], 64, axis=0)
    # the maximum alone has 1 / (1 + n / e) of the mass: top_p = 0.5 needs part of the group, so it takes all of it
    toks, _, kept = check_against_restatement(dev, rows, 8, 3, top_p=0.5)
    assert np.flatnonzero(kept[0]).tolist() == sorted(tie + [5])
    assert len(set(toks.tolist())) > 2
    # min-p at the group's own level keeps it too (e = exp(-1) against min_p = 0.3); top-k = 2 keeps the whole group as well
    _, _, kept = check_against_restatement(dev, rows, 8, 4, top_k=2, top_p=0.9, min_p=0.3)
    assert np.flatnonzero(kept[0]).tolist() == sorted(tie + [5])


@pytest.mark.parametrize("V,M", [(80, 64), (50257, 4)])
def test_off_means_off(dev, V, M):
    """top_p = 1 and min_p = 0 through the new entry: tokens and probs of dg_sample_rows, bit for bit"""
    from drakegpt_amd import ops
    x = torch.from_numpy((np.random.default_rng(V).standard_normal((M, V)) * 3).astype(np.float32)).to(dev)
    for temperature, top_k in ((1.0, None), (0.7, 10), (0.0, None)):
        t0, p0 = ops.sample_rows(x, seed=77, L=12, temperature=temperature, top_k=top_k, probs=True)
        t1, p1 = ops.sample_rows(x, seed=77, L=12, temperature=temperature, top_k=top_k, probs=True, top_p=1.0, min_p=0.0)
        assert torch.equal(t0, t1) and torch.equal(p0, p1)
    # greedy ignores both filters
    tg = ops.sample_rows(x, seed=1, L=0, temperature=0.0, top_p=0.1, min_p=0.9)
    assert torch.equal(tg.cpu(), x.cpu().argmax(1))


@pytest.mark.parametrize("kw", [dict(top_p=0.9), dict(min_p=0.1)])
def test_kernel_frequencies(dev, kw):
    """65536 rows of identical logits: the token frequencies obey the 5-sigma binomial bound against the restatement's p, and no
    token is ever outside the kept set"""
    from drakegpt_amd import ops
    x = torch.randn(80, generator=torch.Generator().manual_seed(3))
    assert_clear(x.numpy()[None], **kw)
    toks = ops.sample_rows(x.repeat(65536, 1).to(dev), seed=1234, L=5, **kw).cpu().numpy()
    p, kept = NM.probs(x.numpy(), **kw)
    assert 1 < kept.sum() < 80
    assert kept[toks].all()
    ok, worst = SM.freq_bound_ok(toks, p)
    print(f"kept {kept.sum()} of 80; worst standardised deviation {worst:.2f} sigma")
    assert ok, worst


# ------------------------------------------------------------------------------------------------------------------ end to end
V = 80
CTX = 32


def lm(dev, precision="fp32"):
    """the model of tests/golden/small_TransformerLM.pt (seed-42 default init)"""
    import drakegpt_amd as D
    torch.manual_seed(42)
    return D.TransformerLM(V, 64, CTX, 4, 2, 0.0, precision=precision).to(dev).eval()


def prompt(dev):
    return torch.tensor([[2, 3]], dtype=torch.long, device=dev)


@torch.no_grad()
def rederive(m, ids, t0, seed, **kw):
    """every token after the prompt, drawn again by the restatement from the full forward's logits on the window before it"""
    ctx = m.context_length
    out = []
    for L in range(t0, ids.shape[1]):
        lo = 0 if ctx is None else max(0, L - ctx)
        logits = m(ids[:, lo:L].contiguous())[0][:, -1].cpu().numpy()
        assert_clear(logits, **kw)
        out.append(NM.sample(logits, seed, L, **kw))
    return np.stack(out, axis=1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_generate_graph_equals_eager(dev, precision):
    m = lm(dev, precision)
    a = m.generate(prompt(dev), 40, sampler="device", top_p=0.9, top_k=20, seed=11)        # 2 + 40 tokens: crosses the window at 32
    assert a.shape == (1, 42) and torch.equal(a[:, :2], prompt(dev))
    from drakegpt_amd.model import Sampling
    b = m._generate_device_cached(prompt(dev), 40, Sampling("device", 1.0, 20, 0.9, seed=11), graph=False)
    assert a.tolist() == b.tolist()
    if precision == "fp32":                             # fp32 decoding is bit-identical to the full forward: re-derive each token
        ref = rederive(m, a, 2, 11, top_k=20, top_p=0.9)
        assert a[:, 2:].cpu().numpy().tolist() == ref.tolist()
        c = m.generate(prompt(dev), 40, sampler="device", top_p=0.9, top_k=20, seed=11, use_cache=False)
        assert c.tolist() == a.tolist()


def test_one_capture_serves_every_setting(dev):
    m = lm(dev)
    a = m.generate(prompt(dev), 40, sampler="device", top_p=0.9, top_k=20, seed=11)
    (dec,) = m._decoders.values()
    graphs = dec.graphs
    assert graphs is not None and dec.params.numel() == 4
    b = m.generate(prompt(dev), 40, sampler="device", top_p=0.3, seed=11)
    c = m.generate(prompt(dev), 40, sampler="device", min_p=0.2, temperature=1.2, seed=11)
    d = m.generate(prompt(dev), 40, sampler="device", seed=11)
    assert list(m._decoders.values()) == [dec] and dec.graphs is graphs                    # no new decoder, no new capture
    assert len({str(t.tolist()) for t in (a, b, c, d)}) == 4
    assert b[:, 2:].cpu().numpy().tolist() == rederive(m, b, 2, 11, top_p=0.3).tolist()
    assert c[:, 2:].cpu().numpy().tolist() == rederive(m, c, 2, 11, min_p=0.2, temperature=1.2).tolist()
    assert d[:, 2:].cpu().numpy().tolist() == rederive(m, d, 2, 11).tolist()               # filters off again: the plain sampler


def test_host_sampler_draws_from_the_kept_set(dev):
    m = lm(dev)
    torch.manual_seed(3)
    h = m.generate(prompt(dev), 40, top_p=0.5, min_p=0.05)
    assert h.shape == (1, 42)
    narrowed = 0
    with torch.no_grad():
        for L in range(2, 42):
            logits = m(h[:, max(0, L - CTX):L].contiguous())[0][:, -1].cpu().numpy()
            assert_clear(logits, top_p=0.5, min_p=0.05)
            _, kept = NM.weights(logits, top_p=0.5, min_p=0.05)
            assert kept[0, int(h[0, L])], L
            narrowed += int(kept.sum() < V)
    assert narrowed == 40
    # and the uncached host path (use_cache=False) takes the same arguments
    torch.manual_seed(3)
    assert m.generate(prompt(dev), 40, top_p=0.5, min_p=0.05, use_cache=False).tolist() == h.tolist()


def test_smaller_model_device_sampler(dev):
    import drakegpt_amd as D
    torch.manual_seed(0)
    m = D.ResidualBlocksLM(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=3).to(dev).eval()
    kw = dict(top_p=0.8, min_p=0.02, temperature=0.9)
    a = m.generate(prompt(dev), 20, sampler="device", seed=31, **kw)
    assert a.tolist() == m.generate(prompt(dev), 20, sampler="device", seed=31, **kw).tolist()
    assert a.tolist() != m.generate(prompt(dev), 20, sampler="device", seed=31).tolist()
    assert a[:, 2:].cpu().numpy().tolist() == rederive(m, a, 2, 31, **kw).tolist()
