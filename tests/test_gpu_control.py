"""GPU: dg_sample_rows_control (repetition / presence / frequency penalties, logit bias, stop tokens inside the sampler kernel) and
dg_token_counts; generate() with the controls end to end: graph-replayed, eager, uncached, host sampler, BigramLM.

Kernel against itself: the new entry on (logits, counts, bias) must equal dg_sample_rows_nucleus on the row adjusted by
tests/control_model.adjust -- four correctly rounded fp32 operations that numpy restates bit for bit -- so tokens and probs are
compared with torch.equal and no margin is needed.  Kernel against the restatement: as in test_gpu_nucleus.py, the kept set
exactly and the tokens equal, after asserting on the restatement alone (assert_clear, on the adjusted row) that every row is
1e-8 away from a decision that the last bit of an fp64 exp could turn; no row is excluded.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_model as CM  # noqa: E402
import nucleus_model as NM  # noqa: E402
import sampling_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu

V = 80
CTX = 32


def lm(dev, precision="fp32"):
    """the tiny model of test_gpu_nucleus.py (tests/golden/small_TransformerLM.pt: seed-42 default init)"""
    import drakegpt_amd as D
    torch.manual_seed(42)
    return D.TransformerLM(V, 64, CTX, 4, 2, 0.0, precision=precision).to(dev).eval()


def assert_clear(x, temperature=1.0, top_k=None, top_p=None, min_p=None):
    """the precondition of an exact comparison, stated on the restatement alone (the margins of test_gpu_nucleus.py)"""
    mg, mm = NM.margins(x, temperature, top_k, top_p, min_p)
    assert (mg >= NM.MARGIN).all(), mg.min()
    assert (mm >= NM.MARGIN).all(), mm.min()


NINF = float("-inf")
POISON = torch.tensor([float("nan"), float("inf"), 1e30, float("nan"), float("inf"), 1e30, float("nan")])


def padded_logits(dev, x):
    """x fp32 numpy [M, V] inside a wider buffer whose padding (NaN, inf, 1e30) must never be read"""
    M, Vx = x.shape
    buf = torch.empty((M, Vx + 7), dtype=torch.float32)
    buf[:, Vx:] = POISON
    buf[:, :Vx] = torch.from_numpy(x)
    return buf.to(dev)[:, :Vx]


def padded_counts(dev, counts):
    """counts int32 numpy [M, V] with ldc = V + 5 and huge padding"""
    M, Vx = counts.shape
    buf = torch.full((M, Vx + 5), 2 ** 30, dtype=torch.int32)
    buf[:, Vx:] = torch.tensor([2 ** 31 - 1, -(2 ** 31), 12345, -1, 2 ** 30])
    buf[:, :Vx] = torch.from_numpy(counts)
    return buf.to(dev)[:, :Vx]


def control(dev, rep=1.0, presence=0.0, frequency=0.0, bias=None, stop=(), pad=None):
    from drakegpt_amd import ops
    return ops.new_sample_control(repetition_penalty=rep, presence_penalty=presence, frequency_penalty=frequency, stop_tokens=stop,
                                  pad_token=pad, use_bias=bias is not None, device=dev)


# ------------------------------------------------------------------------------------------------------- kernel against itself
SHAPES = [(80, 64), (257, 64), (8192, 16), (8193, 16), (50257, 4)]
SETTINGS = [dict(), dict(top_k=20), dict(top_p=0.9), dict(min_p=0.05), dict(temperature=0.7, top_k=50, top_p=0.8), dict(temperature=0.0)]


def random_inputs(Vx, M, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((M, Vx)) * 3).astype(np.float32)
    counts = CM.COUNT_VALUES[g.integers(0, CM.COUNT_VALUES.size, size=(M, Vx))]
    bias = np.zeros(Vx, dtype=np.float32)
    pick = g.permutation(Vx)[:12]
    bias[pick[:4]], bias[pick[4:8]], bias[pick[8:]] = -np.inf, 2.0, -2.0
    return x, counts, bias


@pytest.mark.parametrize("Vx,M", SHAPES)
def test_control_equals_nucleus_on_the_adjusted_row(dev, Vx, M):
    from drakegpt_amd import ops
    x, counts, bias = random_inputs(Vx, M, Vx)
    xd, cd, bd = padded_logits(dev, x), padded_counts(dev, counts), torch.from_numpy(bias).to(dev)
    before = cd.clone()
    for n, (rep, presence, frequency, use_bias) in enumerate(((1.3, 0.0, 0.0, False), (0.8, 0.5, 0.25, True), (1.0, -0.3, 0.1, True),
                                                              (1.7, 0.0, 0.0, True))):
        y = CM.adjust(x, counts, rep, presence, frequency, bias if use_bias else None)
        yd = padded_logits(dev, y)
        ctl = control(dev, rep, presence, frequency, bias if use_bias else None)
        for kw in SETTINGS:
            t1, p1 = ops.sample_rows(xd, seed=31 + n, L=7, probs=True, control=ctl, bias=bd, counts=cd, **kw)
            t0, p0 = ops.sample_rows(yd, seed=31 + n, L=7, probs=True, top_p=kw.get("top_p", 1.0),
                                     **{k: v for k, v in kw.items() if k != "top_p"})
            assert torch.equal(t1, t0), (rep, presence, frequency, use_bias, kw)
            assert torch.equal(p1, p0), (rep, presence, frequency, use_bias, kw)
            if use_bias:
                assert not p1.cpu().numpy()[:, np.isneginf(bias)].any()
            # the token-writing launch counted its token: put the counts back for the next setting
            after = cd.clone()
            after[torch.arange(M, device=dev), t1] -= 1
            assert torch.equal(after, before)
            cd.copy_(before)
        assert torch.equal(cd.cpu(), torch.from_numpy(counts))
    # the padding of counts is as it was
    full = cd.as_strided((M, Vx + 5), (Vx + 5, 1))
    assert full[:, Vx:].cpu().tolist() == [[2 ** 31 - 1, -(2 ** 31), 12345, -1, 2 ** 30]] * M


@pytest.mark.parametrize("i", range(len(CM.CASES)))
def test_control_matches_restatement(dev, i):
    from drakegpt_amd import ops
    Vx, M, temperature, top_k, top_p, min_p, rep, presence, frequency, _ = CM.CASES[i]
    x, counts, bias = CM.case_inputs(i)
    y = CM.adjust(x, counts, rep, presence, frequency, bias)
    kw = dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p)
    assert_clear(y, **kw)
    toks, p_gpu = ops.sample_rows(padded_logits(dev, x), seed=4321, L=3 + i, probs=True, control=control(dev, rep, presence, frequency, bias),
                                  bias=torch.from_numpy(bias).to(dev), counts=padded_counts(dev, counts), **kw)
    toks, p_gpu = toks.cpu().numpy(), p_gpu.cpu().numpy().astype(np.float64)
    p, kept = NM.probs(y, **kw)
    print(f"kept per row: {kept.sum(1).min()} .. {kept.sum(1).max()} of {Vx}")
    assert ((p_gpu > 0) == kept).all()
    assert (kept.sum(1) < Vx).all() and not kept[:, np.isneginf(bias)].any()
    rel = np.abs(p_gpu - p)[kept] / p[kept]
    print(f"probs: max relative error {rel.max():.2e}")
    assert rel.max() <= 1e-6
    ref = CM.sample(x, 4321, 3 + i, counts, rep, presence, frequency, bias, **kw)
    assert (toks == ref).all(), np.flatnonzero(toks != ref)


@pytest.mark.parametrize("Vx,M", [(80, 64), (50257, 4)])
def test_controls_off_means_off(dev, Vx, M):
    """rep = 1, penalties 0, no bias, no stop token, with counts present and non-zero: dg_sample_rows_nucleus bit for bit"""
    from drakegpt_amd import ops
    x, counts, bias = random_inputs(Vx, M, 7 + Vx)
    xd, bd = padded_logits(dev, x), torch.from_numpy(bias).to(dev)
    ctl = control(dev)
    assert ctl.tolist()[4:6] == [0, 0]
    for kw in (dict(), dict(temperature=0.7, top_k=10), dict(top_p=0.9, min_p=0.02), dict(temperature=0.0)):
        t0, p0 = ops.sample_rows(xd, seed=77, L=12, probs=True, top_p=kw.get("top_p", 1.0), **{k: v for k, v in kw.items() if k != "top_p"})
        t1, p1 = ops.sample_rows(xd, seed=77, L=12, probs=True, control=ctl, bias=bd, counts=padded_counts(dev, counts), **kw)
        assert torch.equal(t0, t1) and torch.equal(p0, p1), kw
        t2, p2 = ops.sample_rows(xd, seed=77, L=12, probs=True, control=ctl, **kw)          # and without counts / bias at all
        assert torch.equal(t0, t2) and torch.equal(p0, p2), kw


# ----------------------------------------------------------------------------------------------------------------- bookkeeping
def test_counts_lengths_and_finished_rows(dev):
    from drakegpt_amd import ops
    Vx, M, cap, L = 300, 6, 12, 5
    g = np.random.default_rng(11)
    x = (g.standard_normal((M, Vx)) * 3).astype(np.float32)
    counts = CM.COUNT_VALUES[g.integers(0, 6, size=(M, Vx))]
    # what the rows draw without any stop token
    plain = ops.sample_rows(padded_logits(dev, x), seed=5, L=L, control=control(dev, 1.3), counts=padded_counts(dev, counts)).cpu()
    assert (plain.numpy() == CM.sample(x, 5, L, counts, 1.3)).all()
    stop = (int(plain[1]), int(plain[4]), Vx - 1 if Vx - 1 not in plain.tolist() else Vx - 2)
    hits = [int(t) in stop for t in plain.tolist()]
    assert hits[1] and hits[4] and not all(hits)
    ctl = control(dev, 1.3, stop=stop, pad=17)
    state = ops.new_rng_state(5, dev, step=L)
    ids = torch.full((M, cap), -7, dtype=torch.int64, device=dev)
    lengths = torch.zeros(M, dtype=torch.int32, device=dev)
    lengths[2] = 4                                              # row 2 arrives finished ...
    xn = x.copy()
    xn[2] = np.nan                                              # ... and is indifferent to its logits
    cd = padded_counts(dev, counts)
    ops.sample_rows(padded_logits(dev, xn), state, ids=ids, control=ctl, counts=cd, lengths=lengths)
    want_ids = torch.full((M, cap), -7, dtype=torch.int64)
    want_ids[:, L] = plain
    want_ids[2, L] = 17
    assert torch.equal(ids.cpu(), want_ids)
    want_counts = counts.copy()
    for m in range(M):
        if m != 2:
            want_counts[m, int(plain[m])] += 1
    assert (cd.cpu().numpy() == want_counts).all()
    want_len = [L + 1 if (hits[m] and m != 2) else 0 for m in range(M)]
    want_len[2] = 4
    assert lengths.cpu().tolist() == want_len
    # L >= ld_ids: nothing at all is written
    ids2, len2, cd2 = ids.clone(), lengths.clone(), cd.clone()
    ops.sample_rows(padded_logits(dev, x), ops.new_rng_state(5, dev, step=cap), ids=ids, control=ctl, counts=cd, lengths=lengths)
    ops.sample_rows(padded_logits(dev, x), ops.new_rng_state(5, dev, step=cap + 3), ids=ids, control=ctl, counts=cd, lengths=lengths)
    assert torch.equal(ids, ids2) and torch.equal(lengths, len2) and torch.equal(cd, cd2)
    # probs only: counts are read, never written
    p = ops.sample_rows(padded_logits(dev, x), tokens=False, probs=True, control=ctl, counts=cd)
    assert torch.equal(cd, cd2)
    assert np.abs(p.cpu().numpy() - CM.probs(x, cd2.cpu().numpy(), 1.3)[0]).max() <= 1e-6
    # tokens returned as a vector (ld_ids == 0) count too; lengths are refused there by the wrapper and by the entry
    t = ops.sample_rows(padded_logits(dev, x), seed=5, L=L, control=ctl, counts=cd)
    delta = (cd - cd2).cpu()
    assert delta.sum() == M and (delta[torch.arange(M), t.cpu()] == 1).all()
    with pytest.raises(RuntimeError):
        ops.sample_rows(padded_logits(dev, x), seed=5, L=L, control=ctl, lengths=lengths)


@pytest.mark.parametrize("Vx", [80, 50257])
@pytest.mark.parametrize("n", [1, 5, 300])
def test_token_counts_equals_bincount(dev, Vx, n):
    from drakegpt_amd import ops
    M, cap = 5, 320
    g = np.random.default_rng(n + Vx)
    ids = g.integers(0, Vx, size=(M, cap))
    ids[0, 0], ids[1, 0], ids[2, n - 1] = -3, Vx + 10, 2 ** 40          # clamped as the embedding clamps
    idd = torch.from_numpy(ids).to(dev)
    want = CM.count_prefix(ids[:, :n], Vx)
    buf = torch.full((M, Vx + 3), 99, dtype=torch.int32, device=dev)
    c = ops.token_counts(idd, n, Vx, buf[:, :Vx])                       # zeroing, ldc > V
    assert (c.cpu().numpy() == want).all() and (buf[:, Vx:] == 99).all()
    ops.token_counts(idd, n, Vx, c, accumulate=True)
    assert (c.cpu().numpy() == 2 * want).all() and (buf[:, Vx:] == 99).all()
    ops.token_counts(idd[:, 7:8], 1, Vx, c, accumulate=True)            # one column of a wider buffer
    assert (c.cpu().numpy() == 2 * want + CM.count_prefix(ids[:, 7:8], Vx)).all()
    assert (ops.token_counts(idd, n, Vx).cpu().numpy() == want).all()
    assert int(ops.token_counts(idd, 0, Vx).abs().sum()) == 0


def test_control_frequencies(dev):
    """65536 rows of identical logits and counts with a frequency penalty: the token frequencies obey the 5-sigma binomial bound
    against the restatement's p"""
    from drakegpt_amd import ops
    x = torch.randn(80, generator=torch.Generator().manual_seed(3)).numpy()
    counts = CM.COUNT_VALUES[np.random.default_rng(3).integers(0, 6, size=80)]
    y = CM.adjust(x, counts, frequency=0.4)
    assert_clear(y[None], top_p=0.95)
    N = 65536
    toks = ops.sample_rows(torch.from_numpy(x).repeat(N, 1).to(dev), seed=1234, L=5, top_p=0.95, control=control(dev, frequency=0.4),
                           counts=torch.from_numpy(counts).repeat(N, 1).to(dev)).cpu().numpy()
    p, kept = NM.probs(y, top_p=0.95)
    p_plain, _ = NM.probs(x, top_p=0.95)
    assert 1 < kept.sum() < 80 and kept[toks].all()
    assert np.abs(p - p_plain).max() > 0.01                       # the penalty moved the distribution by far more than the bound resolves
    ok, worst = SM.freq_bound_ok(toks, p)
    print(f"kept {kept.sum()} of 80; worst standardised deviation {worst:.2f} sigma")
    assert ok, worst


# ------------------------------------------------------------------------------------------------------------------ end to end
T0, NEW = 2, 40
BAN = 11


def prompts(dev, B=1):
    return torch.tensor([[2, 3], [5, 7], [1, 4]][:B], dtype=torch.long, device=dev)


PEN = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={BAN: NINF, 20: 1.5}, top_k=30, top_p=0.95)


def restated(m, idx, seed, n_new=NEW, stop=(), pad=None, **kw):
    """control_model.generate on the model's full forward (the cropped window, as the reference)"""
    kw = dict(kw)
    bias = None
    if kw.get("logit_bias") is not None:
        bias = np.zeros(V, dtype=np.float32)
        for k, v in kw["logit_bias"].items():
            bias[k] = v
    kw.pop("logit_bias", None)
    pen = dict(rep=kw.pop("repetition_penalty", 1.0), presence=kw.pop("presence_penalty", 0.0), frequency=kw.pop("frequency_penalty", 0.0))

    def logits_fn(ids):
        with torch.no_grad():
            t = torch.from_numpy(ids[:, -CTX:]).to(idx.device)
            out = m(t.contiguous())[0][:, -1].cpu().numpy()
        y = CM.adjust(out, CM.count_prefix(ids, V), bias=bias, **pen)
        assert_clear(y, **kw)
        return out

    return CM.generate(logits_fn, idx.cpu().numpy(), n_new, V, seed, bias=bias, stop=stop, pad=pad, **pen, **kw)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_generate_with_controls_graph_eager_uncached_restated(dev, precision):
    from drakegpt_amd.model import Sampling, check_control_args
    m = lm(dev, precision)
    idx = prompts(dev)
    a = m.generate(idx, NEW, sampler="device", seed=11, **PEN)                  # 2 + 40 tokens: crosses the window at 32
    assert a.shape == (1, T0 + NEW) and torch.equal(a[:, :T0], idx) and BAN not in a[0, T0:].tolist()
    ctl = check_control_args(1.3, 0.2, 0.1, PEN["logit_bias"], None, None, 64, V)
    b = m._generate_device_cached(idx, NEW, Sampling("device", 1.0, 30, 0.95, ctl=ctl, seed=11), graph=False)
    assert a.tolist() == b.tolist()
    assert a.tolist() != m.generate(idx, NEW, sampler="device", seed=11, top_k=30, top_p=0.95).tolist()
    if precision == "fp32":                             # fp32 decoding is bit-identical to the full forward
        c = m.generate(idx, NEW, sampler="device", seed=11, use_cache=False, **PEN)
        assert c.tolist() == a.tolist()
        assert restated(m, idx, 11, **PEN).tolist() == a.cpu().numpy().tolist()


def test_greedy_frequency_penalty_never_repeats_and_the_ban_holds(dev):
    m = lm(dev)
    idx = prompts(dev)
    plain = m.generate(idx, NEW, sampler="device", temperature=0.0, seed=1)
    ban = int(plain[0, T0])                             # what greedy would say first
    a = m.generate(idx, NEW, sampler="device", temperature=0.0, seed=1, frequency_penalty=1e4, logit_bias={ban: NINF})
    new = a[0, T0:].tolist()
    assert len(set(new)) == NEW and not set(new) & set(idx[0].tolist()) and ban not in new
    assert a.tolist() == m.generate(idx, NEW, sampler="device", temperature=0.0, seed=1, frequency_penalty=1e4, logit_bias={ban: NINF},
                                    use_cache=False).tolist()


def test_one_decoder_two_graph_pairs_every_control_setting(dev):
    m = lm(dev)
    idx = prompts(dev)
    d0 = m.generate(idx, NEW, sampler="device", seed=11)
    (dec,) = m._decoders.values()
    graphs = dec.graphs
    assert graphs is not None and dec.graphs_control is None and dec.params.numel() == 4
    settings = [dict(repetition_penalty=1.5), dict(presence_penalty=0.7, frequency_penalty=0.3, top_p=0.9),
                dict(logit_bias={int(d0[0, T0]): NINF}), dict(stop_tokens=int(d0[0, T0 + 20]), repetition_penalty=1.1, temperature=1.1)]
    outs, second = [], None
    for kw in settings:
        outs.append(m.generate(idx, NEW, sampler="device", seed=11, **kw))
        second = second or dec.graphs_control
        assert second is not None and dec.graphs_control is second          # captured once, on the first call with a control
        assert list(m._decoders.values()) == [dec] and dec.graphs is graphs
    assert len({str(t.tolist()) for t in outs + [d0]}) == 5
    for kw, out in zip(settings, outs):
        kw = dict(kw)
        stop = kw.pop("stop_tokens", None)
        ref = restated(m, idx, 11, stop=() if stop is None else (stop,), **kw)
        assert out.cpu().numpy().tolist() == ref.tolist(), kw
    assert int(d0[0, T0]) not in outs[2][0, T0:].tolist()
    # a call without controls after them: the first pair again, and nothing is inherited -- not even from poisoned buffers
    dec.counts.fill_(1000)
    dec.lengths.fill_(1)
    dec.bias.fill_(NINF)
    d1 = m.generate(idx, NEW, sampler="device", seed=11)
    assert d1.tolist() == d0.tolist() == lm(dev).generate(idx, NEW, sampler="device", seed=11).tolist()
    # and a call with controls after the poison equals the same call on a fresh model
    e = m.generate(idx, NEW, sampler="device", seed=11, **settings[1])
    assert e.tolist() == outs[1].tolist() == lm(dev).generate(idx, NEW, sampler="device", seed=11, **settings[1]).tolist()
    assert dec.graphs is graphs and dec.graphs_control is second


# ------------------------------------------------------------------------------------------------------------------ stop tokens
def pick_stops(plain):
    """two stop tokens from a plain run [B, T0 + NEW], one from row 0 and one from row 1, so that the rows end at different
    positions and a third row, if there is one, never does; returns (stop tuple, end per row)"""
    rows = plain[:, T0:].tolist()
    B = len(rows)
    for a in range(3, NEW - 8):
        for b in range(a + 4, NEW - 2):
            stop = (rows[0][a], rows[1][b])
            if stop[0] == stop[1] or (B > 2 and set(stop) & set(rows[2])):
                continue
            ends = [next((T0 + j + 1 for j, t in enumerate(r) if t in stop), T0 + NEW) for r in rows]
            if len(set(ends)) == B:
                return stop, ends
    raise AssertionError("no usable pair of stop tokens in the plain run")


def check_stopped(out, plain, stop, ends, pad):
    out, plain = out.cpu().numpy(), plain.cpu().numpy()
    assert out.shape == (plain.shape[0], max(ends))
    for m, end in enumerate(ends):
        assert (out[m, :min(end, out.shape[1])] == plain[m, :min(end, out.shape[1])]).all(), m
        assert (out[m, end:] == pad).all(), m
        if end < plain.shape[1]:
            assert int(out[m, end - 1]) in stop


def test_stop_tokens_rows_end_at_different_lengths(dev):
    m = lm(dev)
    idx = prompts(dev, 3)
    kw = dict(sampler="device", seed=5, temperature=1.2)
    plain = m.generate(idx, NEW, **kw)
    # rows 0 and 1 stop, row 2 never does: the width stays T0 + NEW
    stop, ends = pick_stops(plain)
    assert ends[2] == T0 + NEW > max(ends[:2])
    pad = next(t for t in range(V) if t not in stop and t not in plain.tolist()[2])
    outs = [m.generate(idx, NEW, stop_tokens=stop, pad_token=pad, stop_poll=poll, **kw) for poll in (1, 7, 1000)]
    check_stopped(outs[0], plain, stop, ends, pad)
    assert outs[0].tolist() == outs[1].tolist() == outs[2].tolist()
    from drakegpt_amd.model import Sampling, check_control_args
    ctl = check_control_args(1.0, 0.0, 0.0, None, stop, pad, 7, V)
    assert m._generate_device_cached(idx, NEW, Sampling("device", 1.2, ctl=ctl, seed=5), graph=False).tolist() == outs[0].tolist()
    assert m.generate(idx, NEW, stop_tokens=stop, pad_token=pad, stop_poll=7, use_cache=False, **kw).tolist() == outs[0].tolist()
    # the default pad is the first stop token
    d = m.generate(idx, NEW, stop_tokens=stop, **kw)
    check_stopped(d, plain, stop, ends, stop[0])
    # every row stops (a batch of two, stop tokens from its own plain run): trimmed to the longest of them, the same for every
    # poll, graph, eager and uncached
    plain2 = m.generate(idx[:2], NEW, **kw)
    stop, ends = pick_stops(plain2)
    ctl = check_control_args(1.0, 0.0, 0.0, None, stop, pad, 7, V)
    two = [m.generate(idx[:2], NEW, stop_tokens=stop, pad_token=pad, stop_poll=poll, **kw) for poll in (1, 7, 1000)]
    check_stopped(two[0], plain2, stop, ends, pad)
    assert two[0].shape[1] == max(ends) < T0 + NEW
    assert two[0].tolist() == two[1].tolist() == two[2].tolist()
    assert m._generate_device_cached(idx[:2], NEW, Sampling("device", 1.2, ctl=ctl, seed=5), graph=False).tolist() == two[0].tolist()
    assert m.generate(idx[:2], NEW, stop_tokens=stop, pad_token=pad, use_cache=False, **kw).tolist() == two[0].tolist()


@pytest.mark.parametrize("use_cache", [True, False])
def test_host_sampler_stop_tokens_and_penalties(dev, use_cache):
    m = lm(dev)
    idx = prompts(dev, 3)
    plain = m.generate(idx, NEW, torch.Generator().manual_seed(3), use_cache=use_cache)
    stop, ends = pick_stops(plain)
    pad = next(t for t in range(V) if t not in stop and t not in plain.tolist()[2])
    out = m.generate(idx, NEW, torch.Generator().manual_seed(3), use_cache=use_cache, stop_tokens=stop, pad_token=pad)
    check_stopped(out, plain, stop, ends, pad)
    plain2 = m.generate(idx[:2], NEW, torch.Generator().manual_seed(3), use_cache=use_cache)
    stop, ends = pick_stops(plain2)
    two = m.generate(idx[:2], NEW, torch.Generator().manual_seed(3), use_cache=use_cache, stop_tokens=stop, pad_token=pad)
    check_stopped(two, plain2, stop, ends, pad)
    assert two.shape[1] == max(ends) < T0 + NEW
    # with a ban and a huge frequency penalty the host sampler never repeats and never draws the banned token
    h = m.generate(idx, NEW, torch.Generator().manual_seed(3), use_cache=use_cache, temperature=0.0, frequency_penalty=1e4,
                   logit_bias={BAN: NINF})
    for r, p in zip(h.tolist(), idx.tolist()):
        assert len(set(r[T0:])) == NEW and not set(r[T0:]) & set(p) and BAN not in r[T0:]
    # greedy is the same on both samplers
    assert h.tolist() == m.generate(idx, NEW, sampler="device", seed=1, temperature=0.0, frequency_penalty=1e4,
                                    logit_bias={BAN: NINF}).tolist()


def test_bigram_smoke_both_samplers(dev):
    import drakegpt_amd as D
    torch.manual_seed(0)
    m = D.BigramLM(V).to(dev).eval()
    idx = prompts(dev, 2)
    kw = dict(repetition_penalty=1.2, frequency_penalty=0.5, logit_bias={BAN: NINF})
    plain = m.generate(idx, 30, sampler="device", seed=3, **kw)
    assert plain.shape == (2, 32) and BAN not in plain[:, T0:].tolist()[0] + plain[:, T0:].tolist()[1]
    stop = int(plain[0, 12])
    a = m.generate(idx, 30, sampler="device", seed=3, stop_tokens=stop, stop_poll=4, **kw)
    first = [next((T0 + j + 1 for j, t in enumerate(r[T0:]) if t == stop), 32) for r in plain.tolist()]
    check_stopped(a, plain, (stop,), first, stop)
    h = m.generate(idx, 30, torch.Generator().manual_seed(1), stop_tokens=stop, **kw)
    assert h.shape[0] == 2 and T0 < h.shape[1] <= 32 and BAN not in h[:, T0:].flatten().tolist()
    assert h.tolist() == m.generate(idx, 30, torch.Generator().manual_seed(1), stop_tokens=stop, **kw).tolist()
