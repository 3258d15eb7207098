"""GPU: generate(return_logprobs=, top_logprobs=, best_of=) and score() end to end, on the tiny TransformerLM of the generate tests
(V 80, C 64, ctx 32, 4 heads, 2 layers, seed 42): 40 new tokens after a prompt of 2, so every cached case crosses into the
sliding-window phase at 32.

Against the CPU oracle (oracle/drake_ref.py) nothing is compared with a constant: log-softmax moves by at most twice the sup-norm
change of its input, so with e = the largest |logits_gpu - logits_oracle| measured here, on the very windows the numbers were made
from, |lp_gpu - lp_oracle| <= 2 e + 2^-23 max(|lp|, 1) -- the second term is the fp32 rounding of x - m* and of the result.
fp32: the graph-replayed path (its cached steps are bit-identical to the full forward, tests/test_gpu_decode.py, so the forward's
logits are the ones that were scored).  bf16: the uncached device path, whose logits ARE the forward's.
"""
import contextlib
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_model as LM  # noqa: E402

pytestmark = pytest.mark.gpu

V, CTX, T0, NEW = 80, 32, 2, 40
PAD = 79
SEED = 11


def lm(dev, precision="fp32"):
    import drakegpt_amd as D
    torch.manual_seed(42)
    return D.TransformerLM(V, 64, CTX, 4, 2, 0.0, precision=precision).to(dev).eval()


def prompt(dev, B=1, t0=T0):
    return torch.stack([(torch.arange(t0, dtype=torch.long) * 7 + 2 + 5 * b).remainder(V) for b in range(B)]).to(dev).contiguous()


@contextlib.contextmanager
def recording(calls):
    """the launch counter of tests/test_gpu_generate_launches.py: every library call goes through ops.check"""
    from drakegpt_amd import ops
    check = ops.check

    def counting(rc, what):
        calls.append(what)
        return check(rc, what)

    ops.check = counting
    try:
        yield
    finally:
        ops.check = check


MODES = {"plain": {}, "control": dict(repetition_penalty=1.3), "ragged": dict(prompt_lengths=[2, 4, 3], pad_token=PAD)}


def _idx(dev, mode):
    if mode == "ragged":
        return prompt(dev, 3, 4)
    return prompt(dev, 3)


@pytest.fixture(scope="module")
def model(dev):
    return lm(dev)


@pytest.mark.parametrize("mode", list(MODES))
def test_device_sampler_tokens_unchanged_graph_equals_eager_and_unscored_replays_original(dev, model, mode):
    m, kw = model, dict(MODES[mode], sampler="device", seed=SEED, temperature=0.9, top_k=30)
    idx = _idx(dev, mode)
    plain = m.generate(idx, NEW, **kw)
    dec = next(iter(m._decoders.values()))
    before = dict(dec.pairs)
    assert mode not in dec.pairs_scored
    gen = m.generate(idx, NEW, return_logprobs=True, top_logprobs=3, **kw)
    assert type(gen).__name__ == "Generation" and torch.equal(gen.ids, plain)
    assert mode in dec.pairs_scored and dict(dec.pairs) == before             # twins captured lazily, the originals untouched
    assert gen.logprobs.shape == gen.ids.shape and gen.logprobs.dtype == torch.float32
    assert gen.top_ids.shape == gen.ids.shape + (3,) and gen.top_logprobs.shape == gen.ids.shape + (3,)
    # an unscored call after a scored one replays the original graphs: the same launches as before, the same tokens
    a, b = [], []
    with recording(a):
        again = m.generate(idx, NEW, **kw)
    assert torch.equal(again, plain) and dict(dec.pairs) == before
    assert "dg_token_logprobs" not in a
    # graph path == eager path, bit for bit
    eager = m._generate_device_cached(*_entered(m, idx, kw, return_logprobs=True, top_logprobs=3), graph=False)
    for x, y in zip(gen, eager):
        assert torch.equal(x, y)
    # and == the uncached device loop (fp32: the cached steps are bit-identical to the full forward)
    unc = m.generate(idx, NEW, use_cache=False, return_logprobs=True, top_logprobs=3, **kw)
    for x, y in zip(gen, unc):
        assert torch.equal(x, y)
    # generated positions are scored (finite, <= 0), everything else is 0.0 / -1 / -inf
    first = torch.tensor(kw.get("prompt_lengths", [T0] * 3), device=dev)
    pos = torch.arange(gen.ids.shape[1], device=dev)[None]
    made = (pos >= first[:, None]) & (pos < gen.lengths[:, None])
    assert (gen.logprobs[made] < 0).all() and torch.isfinite(gen.logprobs[made]).all() and (gen.logprobs[~made] == 0).all()
    assert (gen.top_ids[made] >= 0).all() and (gen.top_ids[~made] == -1).all() and torch.isinf(gen.top_logprobs[~made]).all()
    # top-1 is at least as likely as the sampled token, and equal where the sampled token is the top one
    assert (gen.top_logprobs[made][:, 0] >= gen.logprobs[made]).all()
    same = gen.top_ids[made][:, 0].long() == gen.ids[made]
    assert torch.equal(gen.top_logprobs[made][:, 0][same], gen.logprobs[made][same])


def _entered(m, idx, kw, **extra):
    """what generate() hands to the cached loop: (idx after Sampling.enter, max_new_tokens, the checked request)"""
    from drakegpt_amd.model import Sampling
    kw = dict(kw)
    args = dict(generator=None, sampler=kw.pop("sampler"), temperature=kw.pop("temperature", 1.0), top_k=kw.pop("top_k", None),
                seed=kw.pop("seed"), top_p=None, min_p=None, repetition_penalty=kw.pop("repetition_penalty", 1.0), presence_penalty=0.0,
                frequency_penalty=0.0, logit_bias=None, stop_tokens=kw.pop("stop_tokens", None), pad_token=kw.pop("pad_token", None),
                stop_poll=64, prompt_lengths=kw.pop("prompt_lengths", None), shape=tuple(idx.shape))
    assert not kw
    req = Sampling.checked(V, **args, **extra)
    idx, done = req.enter(idx, NEW)
    assert done is None
    return idx, NEW, req


@pytest.mark.parametrize("mode", list(MODES))
def test_host_sampler_tokens_unchanged(dev, model, mode):
    kw = dict(MODES[mode])
    idx = _idx(dev, mode)
    plain = model.generate(idx, NEW, torch.Generator().manual_seed(3), **kw)
    gen = model.generate(idx, NEW, torch.Generator().manual_seed(3), return_logprobs=True, **kw)
    assert torch.equal(gen.ids, plain)
    sc = model.score(gen.ids[:, :CTX + 1])
    first = kw.get("prompt_lengths", [T0] * 3)
    for b in range(3):
        hi = min(int(gen.lengths[b]), CTX + 1)
        assert torch.equal(gen.logprobs[b, first[b]:hi], sc.logprobs[b, first[b] - 1:hi - 1])          # generate's numbers are score()'s


def test_a_scored_step_has_exactly_one_launch_more(dev, model):
    idx = prompt(dev)
    kw = dict(sampler="device", seed=SEED)
    for cached in (True, False):
        a, b = [], []
        if cached:
            with recording(a):
                model._generate_device_cached(*_entered(model, idx, kw), graph=False)
            with recording(b):
                model._generate_device_cached(*_entered(model, idx, kw, return_logprobs=True), graph=False)
        else:
            with recording(a):
                model.generate(idx, NEW, use_cache=False, **kw)
            with recording(b):
                model.generate(idx, NEW, use_cache=False, return_logprobs=True, **kw)
        assert b.count("dg_token_logprobs") == NEW and len(b) == len(a) + NEW          # one per step, the prefill's tail included
        assert [c for c in b if c != "dg_token_logprobs"] == a
        at = [i for i, c in enumerate(b) if c == "dg_token_logprobs"]
        assert all(b[i - 1].startswith("dg_sample_rows") and b[i + 1] == "dg_state_advance" for i in at)


def test_ragged_rows_equal_their_own_calls(dev, model):
    kw = dict(sampler="device", seed=SEED, pad_token=PAD, return_logprobs=True, top_logprobs=2)
    idx, first = prompt(dev, 3, 4), [2, 4, 3]
    gen = model.generate(idx, NEW, prompt_lengths=first, **kw)
    for b in range(3):
        # prompt b alone IN THAT ROW: rows 0..b-1 are fillers (the draw is keyed by (seed, position, row))
        alone = idx[b:b + 1, :first[b]].repeat(b + 1, 1).contiguous()
        one = model.generate(alone, NEW, prompt_lengths=[first[b]] * (b + 1), **kw)
        n = first[b] + NEW
        assert torch.equal(one.ids[b], gen.ids[b, :n])
        assert torch.equal(one.logprobs[b], gen.logprobs[b, :n]) and torch.equal(one.top_ids[b], gen.top_ids[b, :n])
        assert (gen.logprobs[b, n:] == 0).all() and (gen.logprobs[b, :first[b]] == 0).all()


@pytest.mark.parametrize("sampler", ["device", "host"])
def test_stop_token_is_scored_and_padding_is_zero(dev, model, sampler):
    idx = prompt(dev, 2)
    args = (torch.Generator().manual_seed(5),) if sampler == "host" else ()
    kw = dict(sampler="device", seed=SEED) if sampler == "device" else {}
    plain = model.generate(idx, NEW, *args, **kw)
    stop = int(plain[0, T0 + 9])                                           # row 0's 10th new token
    args = (torch.Generator().manual_seed(5),) if sampler == "host" else ()
    gen = model.generate(idx, NEW, *args, stop_tokens=stop, pad_token=PAD, return_logprobs=True, top_logprobs=1, **kw)
    n0 = int(gen.lengths[0])
    assert n0 <= T0 + 10 and int(gen.ids[0, n0 - 1]) == stop
    for b in range(2):
        n = int(gen.lengths[b])
        assert torch.equal(gen.ids[b, :n], plain[b, :n])
        assert (gen.logprobs[b, T0:n] < 0).all()                           # the stop token's own position included
        assert (gen.logprobs[b, n:] == 0).all() and (gen.top_ids[b, n:] == -1).all() and (gen.ids[b, n:] == PAD).all()
    sc = model.score(gen.ids[:, :n0])
    assert torch.equal(sc.logprobs[0, T0 - 1:], gen.logprobs[0, T0:n0]), (sc.logprobs[0, T0 - 1:] - gen.logprobs[0, T0:n0]).abs().max()


# ------------------------------------------------------------------------------------------------------------------ the oracle
def _oracle_windows(m, ids, bf16):
    """per generated position j >= T0: (GPU logits, oracle logits) of the very window position j was sampled from,
    ids[:, max(0, j - ctx):j] -- the call the uncached loop makes, one forward each"""
    from oracle import drake_ref as R
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    cpu = ids.cpu()
    g, o = [], []
    with torch.no_grad():
        for j in range(T0, ids.shape[1]):
            lo = max(0, j - CTX)
            g.append(m(ids[:, lo:j].contiguous())[0][:, -1:])
            o.append(R.lm_forward("TransformerLM", sd, cpu[:, lo:j], bf16=bf16)[0][:, -1:])
    return torch.cat(g, 1).cpu().double(), torch.cat(o, 1).double()          # (B, n - T0, V): row i predicts position T0 + i


def _bound(e, lp):
    return 2 * e + 2.0 ** -23 * lp.abs().clamp(min=1)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_generate_and_score_against_the_oracle(dev, precision):
    m = lm(dev, precision)
    bf16 = precision == "bf16"
    idx = prompt(dev, 2)
    gen = m.generate(idx, NEW, sampler="device", seed=SEED, use_cache=not bf16, return_logprobs=True)
    ids = gen.ids
    assert ids.shape[1] == T0 + NEW > CTX + 1                              # the sliding-window phase is in
    lg, lo = _oracle_windows(m, ids, bf16)
    e = (lg - lo).abs().max().item()
    ref = torch.log_softmax(lo, -1).gather(2, ids[:, T0:].cpu()[:, :, None])[:, :, 0]
    got = gen.logprobs[:, T0:].cpu().double()
    err = (got - ref).abs()
    print(f"{precision}: e = {e:.3e}, generate lp err {err.max().item():.3e} (bound {_bound(e, ref).min().item():.3e})")
    assert e < 0.1 and (err <= _bound(e, ref)).all()
    # score(): one forward on the first ctx + 1 tokens; its logits are those of the first window above
    sc = m.score(ids[:, :CTX + 1], top_logprobs=2)
    k = CTX + 1 - T0
    full_o = _full_oracle(m, ids[:, :CTX], bf16)
    full_g = m(ids[:, :CTX].contiguous())[0].detach().cpu().double()
    e2 = (full_g - full_o).abs().max().item()
    ref2 = torch.log_softmax(full_o, -1).gather(2, ids[:, 1:CTX + 1].cpu()[:, :, None])[:, :, 0]
    err2 = (sc.logprobs.cpu().double() - ref2).abs()
    print(f"{precision}: e = {e2:.3e}, score lp err {err2.max().item():.3e}")
    assert (err2 <= _bound(e2, ref2)).all()
    if not bf16:
        d = (sc.logprobs[:, T0 - 1:] - gen.logprobs[:, T0:CTX + 1]).abs().max().item()
        assert torch.equal(sc.logprobs[:, T0 - 1:], gen.logprobs[:, T0:CTX + 1]), d          # generate's numbers are score()'s
    assert k == sc.logprobs.shape[1] - (T0 - 1)


def test_score_ranks_accuracy_and_perplexity_against_the_oracle(dev, model):
    """fp32, on LM.rank_case_ids (tests/test_logprobs_host.py shows on the CPU that the oracle leaves at most 5 % of these
    positions within 4 e of a neighbour for any e up to 1e-4): the ranks agree with the oracle's wherever its gap between the
    target and its neighbours in sorted order exceeds 4 e, e measured here"""
    ids = LM.rank_case_ids(V, CTX + 1).to(dev)
    sc = model.score(ids, top_logprobs=2)
    full_o = _full_oracle(model, ids[:, :CTX], False)
    e = (model(ids[:, :CTX].contiguous())[0].detach().cpu().double() - full_o).abs().max().item()
    tgt = ids[:, 1:].cpu()
    clear, rank_o = LM.clear_positions(full_o, tgt, e)
    print(f"e = {e:.3e}, positions compared {clear.float().mean().item():.1%}")
    assert clear.float().mean().item() >= 0.95, clear.float().mean().item()
    assert torch.equal(sc.ranks.cpu().long()[clear], rank_o[clear])
    # accuracy and perplexity follow from the outputs
    assert sc.mask.all()
    assert sc.accuracy(1) == float((sc.ranks == 0).float().mean()) and sc.accuracy(5) >= sc.accuracy(1)
    assert abs(sc.perplexity() - math.exp(-sc.logprobs.double().mean().item())) < 1e-9 * sc.perplexity()
    assert (sc.top_ids[:, :, 0][sc.ranks == 0].long() == ids[:, 1:][sc.ranks == 0]).all()
    assert (sc.top_logprobs[:, :, 0] >= sc.logprobs).all()


def _full_oracle(m, ids, bf16):
    from oracle import drake_ref as R
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        return R.lm_forward("TransformerLM", sd, ids.cpu(), bf16=bf16)[0].double()


def test_score_prompt_lengths_mask(dev, model):
    ids = torch.randint(0, V, (3, 12), generator=torch.Generator().manual_seed(1)).to(dev)
    full = model.score(ids, top_logprobs=2)
    first = [12, 5, 1]
    junk = ids.clone()
    junk[1, 5:], junk[2, 1:] = 10 ** 6, -4                                   # what lies beyond a row's length is read by nothing
    sc = model.score(junk, prompt_lengths=first, top_logprobs=2)
    want = torch.arange(1, 12, device=dev)[None] < torch.tensor(first, device=dev)[:, None]
    assert torch.equal(sc.mask, want)
    for a, b in zip(sc[:4], full[:4]):
        assert torch.equal(a[want], b[want])                                 # the masked positions and nothing else
    assert (sc.logprobs[~want] == 0).all() and (sc.ranks[~want] == -1).all() and (sc.top_ids[~want] == -1).all()
    assert torch.isinf(sc.top_logprobs[~want]).all()
    n = int(want.sum())
    assert abs(sc.perplexity() - math.exp(-sc.logprobs.double().sum().item() / n)) < 1e-9 * sc.perplexity()
    assert sc.accuracy(3) == float(((sc.ranks >= 0) & (sc.ranks < 3)).sum()) / n


def test_score_ignores_train_mode_dropout(dev):
    import drakegpt_amd as D
    torch.manual_seed(42)
    m = D.TransformerLM(V, 64, CTX, 4, 2, 0.2).to(dev)
    ids = torch.randint(0, V, (2, 9), generator=torch.Generator().manual_seed(2)).to(dev)
    a = m.train().score(ids)
    assert m.training
    b = m.eval().score(ids)
    assert torch.equal(a.logprobs, b.logprobs) and torch.equal(a.ranks, b.ranks)


def test_best_of_keeps_the_candidate_with_the_highest_mean_score(dev, model):
    idx, first = prompt(dev, 2, 4), [4, 2]
    kw = dict(sampler="device", seed=SEED, pad_token=PAD, stop_tokens=[7])
    best = model.generate(idx, 12, prompt_lengths=first, best_of=4, **kw)
    assert best.ids.shape[0] == 2
    # the equivalent B * 4-row call: candidate c of prompt b is row 4 b + c
    rep, first4 = idx.repeat_interleave(4, 0), [p for p in first for _ in range(4)]
    cand = model.generate(rep, 12, prompt_lengths=first4, return_logprobs=True, **kw)
    sc = model.score(cand.ids, prompt_lengths=cand.lengths.tolist())
    pos = torch.arange(1, cand.ids.shape[1], device=dev)[None]
    gen_mask = sc.mask & (pos >= torch.tensor(first4, device=dev)[:, None])
    mean = (sc.logprobs.double() * gen_mask).sum(1) / gen_mask.sum(1)
    for b in range(2):
        c = int(mean[4 * b:4 * b + 4].argmax())
        n = int(cand.lengths[4 * b + c])
        assert int(best.lengths[b]) == n and torch.equal(best.ids[b, :n], cand.ids[4 * b + c, :n])
        assert torch.equal(best.logprobs[b, :n], cand.logprobs[4 * b + c, :n]) and (best.ids[b, n:] == PAD).all()
    assert best.ids.shape[1] == int(best.lengths.max())


@pytest.mark.parametrize("name", ["BigramLM", "SingleHeadAttentionLM", "MultiHeadAttentionLM", "BlocksLM", "ResidualBlocksLM", "TransformerLM"])
def test_all_six_models_accept_the_arguments(dev, name):
    import drakegpt_amd as D
    torch.manual_seed(0)
    ctor = {"BigramLM": lambda: D.BigramLM(V), "SingleHeadAttentionLM": lambda: D.SingleHeadAttentionLM(V, 32, 16, 32),
            "MultiHeadAttentionLM": lambda: D.MultiHeadAttentionLM(V, 32, 16, 32, 4), "BlocksLM": lambda: D.BlocksLM(V, 32, 16, 4, 2),
            "ResidualBlocksLM": lambda: D.ResidualBlocksLM(V, 32, 16, 4, 2), "TransformerLM": lambda: D.TransformerLM(V, 32, 16, 4, 2, 0.0)}
    m = ctor[name]().to(dev).eval()
    idx = prompt(dev, 2, 3)
    for sampler in ("host", "device"):
        gen = m.generate(idx, 6, sampler=sampler, return_logprobs=True, top_logprobs=2, best_of=2, pad_token=PAD)
        assert gen.ids.shape == (2, 9) and gen.logprobs.shape == (2, 9) and gen.top_ids.shape == (2, 9, 2)
        sc = m.score(gen.ids)
        assert torch.equal(sc.logprobs[:, 2:], gen.logprobs[:, 3:])
        assert (gen.logprobs[:, :3] == 0).all() and (gen.logprobs[:, 3:] < 0).all()
