"""GPU: generate(sampler="device") -- tokens drawn by dg_sample_rows, the K/V-cached and the sliding-window phase each replayed
as one captured graph -- against a loop written here (full forward per token + ops.sample_rows with the position as a host
integer), against the uncached path, the CPU oracle, and the untouched default (host torch.multinomial) behaviour."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

V = 80


def lm(dev, precision="fp32", seed=0):
    import drakegpt_amd as D
    torch.manual_seed(seed)
    return D.TransformerLM(V, 64, 24, 4, 2, 0.1, precision=precision).to(dev).eval()


def prompt(dev):
    return torch.tensor([[2, 3]], dtype=torch.long, device=dev)


@torch.no_grad()
def loop(m, idx, n, seed, **kw):
    """the reference algorithm (src/model.py:625-635) with the device sampler; returns (ids, the logits each token was drawn from)"""
    from drakegpt_amd import ops
    ctx, used = m.context_length, []
    for _ in range(n):
        L = idx.shape[1]
        cond = idx if ctx is None else idx[:, -ctx:]
        logits = m(cond.contiguous())[0][:, -1]
        used.append(logits)
        tok = ops.sample_rows(logits, seed=seed, L=L, **kw)
        idx = torch.cat((idx, tok[:, None]), dim=1)
    return idx, used


def test_graph_decode_equals_the_loop_and_the_uncached_path(dev):
    m = lm(dev)
    a = m.generate(prompt(dev), 40, sampler="device", seed=11)            # 2 + 40 tokens: crosses the window at 24
    assert a.shape == (1, 42) and a.dtype == torch.int64 and torch.equal(a[:, :2], prompt(dev))
    ref, _ = loop(m, prompt(dev), 40, 11)
    assert a.tolist() == ref.tolist()
    b = m.generate(prompt(dev), 40, sampler="device", seed=11, use_cache=False)
    assert b.tolist() == a.tolist()
    assert m.generate(prompt(dev), 40, sampler="device", seed=11).tolist() == a.tolist()          # replayed again: same tokens
    c = m.generate(prompt(dev), 40, sampler="device", seed=12)
    assert c.tolist() != a.tolist()
    # a prompt that already fills the window starts in the sliding phase; a batch of 3 captures its own graphs
    long = torch.randint(0, V, (3, 30), generator=torch.Generator().manual_seed(1)).to(dev)
    assert m.generate(long, 5, sampler="device", seed=4).tolist() == loop(m, long, 5, 4)[0].tolist()
    short = long[:, :7].contiguous()
    assert m.generate(short, 25, sampler="device", seed=4).tolist() == loop(m, short, 25, 4)[0].tolist()
    # seed=None draws the seed from the CPU generator: reproducible under torch.manual_seed
    torch.manual_seed(77)
    d1 = m.generate(prompt(dev), 12, sampler="device")
    torch.manual_seed(77)
    d2 = m.generate(prompt(dev), 12, sampler="device")
    g = torch.Generator().manual_seed(77)
    d3 = m.generate(prompt(dev), 12, generator=g, sampler="device")
    assert d1.tolist() == d2.tolist() == d3.tolist()


def test_temperature_and_top_k(dev):
    m = lm(dev)
    a = m.generate(prompt(dev), 40, sampler="device", seed=5, temperature=0.8, top_k=5)
    ref, used = loop(m, prompt(dev), 40, 5, temperature=0.8, top_k=5)
    assert a.tolist() == ref.tolist()
    for i, logits in enumerate(used):
        assert int(a[0, 2 + i]) in logits[0].topk(5).indices.tolist()
    # the host sampler with the same filter: torch.multinomial on the filtered distribution
    torch.manual_seed(3)
    h = m.generate(prompt(dev), 40, temperature=0.8, top_k=5)
    with torch.no_grad():
        for L in range(2, 42):
            logits = m(h[:, max(0, L - 24):L].contiguous())[0][0, -1]
            assert int(h[0, L]) in logits.topk(5).indices.tolist()
    # temperature 0 is greedy on both samplers
    g1 = m.generate(prompt(dev), 30, sampler="device", temperature=0)
    g2 = m.generate(prompt(dev), 30, temperature=0)
    assert g1.tolist() == g2.tolist()


def test_greedy_tokens_are_the_oracle_argmax(dev, golden_dir):
    """temperature 0 on the model of tests/golden/small_TransformerLM.pt (seed-42 default init): every chosen token's logit in
    the CPU oracle's full forward is within 1e-5 of that row's maximum (fp32 tracks the oracle to ~2e-7)"""
    import drakegpt_amd as D
    from oracle import drake_ref as R
    fix = torch.load(os.path.join(golden_dir, "small_TransformerLM.pt"), weights_only=True)
    torch.manual_seed(42)
    m = D.TransformerLM(V, 64, 32, 4, 2, 0.0).to(dev).eval()
    with torch.no_grad():
        got = m(fix["T5.x"].to(dev))[0].reshape(-1, V).cpu()
    assert (got - fix["T5.logits"]).abs().max() < 1e-4              # the fixture's model
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    out = m.generate(prompt(dev), 40, sampler="device", temperature=0).cpu()
    assert out.shape == (1, 42)                                     # crosses the 32-token window
    for L in range(2, 42):
        logits, _ = R.lm_forward("TransformerLM", sd, out[:, max(0, L - 32):L])
        row = logits[0, -1]
        assert row[out[0, L]] >= row.max() - 1e-5, (L, float(row.max() - row[out[0, L]]))


def test_bf16_graph_equals_the_eager_cached_steps(dev):
    """both paths launch the same kernels in the same order; the graph only removes the host from between them"""
    m = lm(dev, "bf16")
    a = m.generate(prompt(dev), 40, sampler="device", seed=21)
    from drakegpt_amd.model import Sampling
    b = m._generate_device_cached(prompt(dev), 40, Sampling("device", seed=21), graph=False)
    assert a.tolist() == b.tolist()
    assert m.generate(prompt(dev), 40, sampler="device", seed=22).tolist() != a.tolist()


def test_no_per_token_host_work(dev, monkeypatch):
    """the number of library calls made by generate() does not depend on the number of tokens: the loop is graph replays"""
    from drakegpt_amd import ops
    m = lm(dev)
    m.generate(prompt(dev), 40, sampler="device", seed=1)           # captures both graphs
    calls = []
    real = ops.check

    def counting(rc, what):
        calls.append(what)
        return real(rc, what)

    monkeypatch.setattr(ops, "check", counting)
    m.generate(prompt(dev), 8, sampler="device", seed=1)
    n8 = len(calls)
    m.generate(prompt(dev), 40, sampler="device", seed=1)
    n40 = len(calls) - n8
    assert n8 == n40 and n8 > 0, (n8, n40)
    # the eager loop, for contrast, launches per token
    calls.clear()
    m.generate(prompt(dev), 8, sampler="device", seed=1, use_cache=False)
    assert len(calls) > 8 * 10


def test_weights_updated_between_calls_are_seen(dev):
    m = lm(dev)
    a = m.generate(prompt(dev), 40, sampler="device", seed=9)
    with torch.no_grad():
        m.lm_head.weight.mul_(-1.0)
        m.blocks[0].ffwd.net[0].bias.add_(0.5)
    b = m.generate(prompt(dev), 40, sampler="device", seed=9)
    assert b.tolist() != a.tolist()
    assert b.tolist() == loop(m, prompt(dev), 40, 9)[0].tolist()


def test_defaults_are_untouched(dev):
    """generate(idx, n) with no new keyword: torch.multinomial on the host generator over softmax_rows of the full forward"""
    from drakegpt_amd import ops
    m = lm(dev)
    torch.manual_seed(5)
    a = m.generate(prompt(dev), 40)
    torch.manual_seed(5)
    idx = prompt(dev)
    with torch.no_grad():
        for _ in range(40):
            probs = ops.softmax_rows(m(idx[:, -24:].contiguous())[0][:, -1])
            idx = torch.cat((idx, torch.multinomial(probs.cpu(), num_samples=1).to(dev)), dim=1)
    assert a.tolist() == idx.tolist()


@pytest.mark.parametrize("name,kw", [
    ("ResidualBlocksLM", dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=3)),
    ("BigramLM", dict(vocab_size=V)),
])
def test_smaller_models_device_sampler(dev, name, kw):
    import drakegpt_amd as D
    torch.manual_seed(0)
    m = D.MODEL_CLASSES[name](**kw).to(dev).eval()
    a = m.generate(prompt(dev), 20, sampler="device", seed=31)
    assert a.tolist() == m.generate(prompt(dev), 20, sampler="device", seed=31).tolist()
    assert a.tolist() != m.generate(prompt(dev), 20, sampler="device", seed=32).tolist()
    assert a.tolist() == loop(m, prompt(dev), 20, 31)[0].tolist()
    assert "check_ids" not in m.__dict__                            # the loop's id-check bypass does not outlive the call
