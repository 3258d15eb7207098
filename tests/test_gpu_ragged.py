"""GPU: dg_sample_rows_ragged and dg_token_counts_rows, and generate(prompt_lengths=, return_lengths=) end to end: graph-replayed,
eager, uncached, host sampler, BigramLM.

Kernel against itself: on a row that samples, the new entry must equal dg_sample_rows_control on the same operands bit for bit
(token, probs, counts, lengths), so everything is compared with torch.equal; the only addition is the budget write, which the test
states from the spans.  Forced and finished rows carry NaN logits inside poisoned padding: nothing of them may be read.
Model level: a row of a ragged batch must equal the same row of a rectangular batch made of its own prompt (fp32: cached decoding
is bit-identical to the full forward, tests/test_gpu_models.py), so again token for token and no margin is needed.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_model as CM  # noqa: E402
import ragged_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu

V = 80
CTX = 32
NEW = 40
PAD = 79
NINF = float("-inf")
ERR_ARG = -1
POISON = torch.tensor([float("nan"), float("inf"), 1e30, float("nan"), float("inf"), 1e30, float("nan")])


def lm(dev, precision="fp32"):
    """the tiny model of test_gpu_control.py (seed-42 default init)"""
    import drakegpt_amd as D
    torch.manual_seed(42)
    return D.TransformerLM(V, 64, CTX, 4, 2, 0.0, precision=precision).to(dev).eval()


def padded_logits(dev, x):
    """x fp32 numpy [M, V] inside a wider buffer whose padding (NaN, inf, 1e30) must never be read"""
    M, Vx = x.shape
    buf = torch.empty((M, Vx + 7), dtype=torch.float32)
    buf[:, Vx:] = POISON
    buf[:, :Vx] = torch.from_numpy(x)
    return buf.to(dev)[:, :Vx]


# ------------------------------------------------------------------------------------------------------------------ the kernel
L, CAP = 5, 12
# role -> (span, lengths on arrival); L = 5.  "first": the row's first sampled position is this one (L == first)
SPANS = {"forced": ((L + 2, L + 12), 0), "sample": ((3, 13), 0), "budget": ((2, L + 1), 0), "finished": ((1, 4), 4),
         "stop": ((L, L + 10), 0)}
# at M = 4 the budget row is also the sampling row that draws no stop token
ROLES = {8: ["forced", "sample", "budget", "finished", "stop", "sample", "forced", "budget"], 4: ["forced", "stop", "budget", "finished"]}
KERNEL_SETTINGS = [dict(), dict(temperature=0.7, top_k=20, top_p=0.9, min_p=0.01), dict(temperature=0.0)]


class Operands:
    """one set of device operands of the control / ragged entries, with padded logits and counts and a sentinel in probs"""

    def __init__(self, dev, x, counts, bias, lengths, ids):
        from drakegpt_amd import ops
        M, Vx = x.shape
        self.M, self.V = M, Vx
        self.logits = padded_logits(dev, x)
        self.cbuf = torch.full((M, Vx + 5), 12345, dtype=torch.int32, device=dev)
        self.counts = self.cbuf[:, :Vx]
        self.counts.copy_(torch.from_numpy(counts))
        self.bias = torch.from_numpy(bias).to(dev)
        self.lengths = torch.tensor(lengths, dtype=torch.int32, device=dev)
        self.ids = ids.clone().to(dev)
        self.probs = torch.full((M, Vx + 3), 7.0, dtype=torch.float32, device=dev)
        self.state = ops.new_rng_state(5, dev, step=L)

    def launch(self, name, params, control, spans=None, **null):
        """the raw entry: -> its return code.  null: operands to pass as NULL (or ld_ids=0)"""
        from drakegpt_amd import _lib, ops
        a = dict(logits=self.logits, state=self.state, params=params, ids=self.ids, control=control, bias=self.bias, counts=self.counts,
                 lengths=self.lengths, spans=spans)
        a.update({k: None for k, v in null.items() if v is None})
        p = ops._p
        args = [p(a["logits"]), ops._ld(self.logits), self.M, self.V, p(a["state"]), p(a["params"]), p(a["ids"]),
                null.get("ld_ids", self.ids.shape[1]), p(self.probs), self.probs.shape[1], p(a["control"]), p(a["bias"]), p(a["counts"]),
                ops._ld(self.counts), p(a["lengths"])]
        if name == "dg_sample_rows_ragged":
            args.append(p(a["spans"]))
        rc = getattr(_lib.lib, name)(*args, ops._stream())
        torch.cuda.synchronize()
        return rc

    def snapshot(self):
        return [t.clone() for t in (self.ids, self.cbuf, self.lengths, self.probs)]


def kernel_inputs(Vx, M, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((M, Vx)) * 3).astype(np.float32)
    counts = CM.COUNT_VALUES[g.integers(0, CM.COUNT_VALUES.size, size=(M, Vx))]
    bias = np.zeros(Vx, dtype=np.float32)
    pick = g.permutation(Vx)[:12]
    bias[pick[:4]], bias[pick[4:8]], bias[pick[8:]] = -np.inf, 2.0, -2.0
    ids = torch.from_numpy(g.integers(0, Vx, size=(M, CAP)))               # "prompt tokens" everywhere: a forced row keeps them
    return x, counts, bias, ids


@pytest.mark.parametrize("M", [8, 4])
@pytest.mark.parametrize("Vx", [80, 50257])
def test_one_launch_mixes_forced_sampling_budget_finished_and_stopped_rows(dev, Vx, M):
    from drakegpt_amd import ops
    roles = ROLES[M]
    x, counts, bias, ids = kernel_inputs(Vx, M, 100 + Vx + M)
    spans = torch.tensor([SPANS[r][0] for r in roles], dtype=torch.int32, device=dev)
    lengths = [SPANS[r][1] for r in roles]
    quiet = [m for m, r in enumerate(roles) if r in ("forced", "finished")]
    live = [m for m in range(M) if m not in quiet]
    xn = x.copy()
    xn[quiet] = np.nan                                                     # neither kind of row may read a logit
    for n, kw in enumerate(KERNEL_SETTINGS):
        params = ops.new_sample_params(kw.get("temperature", 1.0), kw.get("top_k"), dev, top_p=kw.get("top_p"), min_p=kw.get("min_p"),
                                       four=True)
        pen = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, use_bias=True, pad_token=17, device=dev)
        # what the rows draw without a stop token: dg_sample_rows_control on the clean logits; the stop rows' tokens become the stops
        ref0 = Operands(dev, x, counts, bias, lengths, ids)
        assert ref0.launch("dg_sample_rows_control", params, ops.new_sample_control(**pen)) == 0
        stop = sorted({int(ref0.ids[m, L]) for m, r in enumerate(roles) if r == "stop"})
        ctl = ops.new_sample_control(stop_tokens=stop, **pen)
        ref = Operands(dev, x, counts, bias, lengths, ids)
        assert ref.launch("dg_sample_rows_control", params, ctl) == 0
        got = Operands(dev, xn, counts, bias, lengths, ids)
        before = got.snapshot()
        assert got.launch("dg_sample_rows_ragged", params, ctl, spans) == 0
        for m, r in enumerate(roles):
            if r == "forced":                          # ids, counts, lengths and the row of probs: bit-unchanged
                for t, b in zip((got.ids, got.cbuf, got.lengths, got.probs), before):
                    assert torch.equal(t[m], b[m]), (m, kw)
            elif r == "finished":                      # pad at L, nothing else
                want = before[0][m].clone()
                want[L] = 17
                assert torch.equal(got.ids[m], want) and int(got.lengths[m]) == 4, (m, kw)
                assert torch.equal(got.cbuf[m], before[1][m]) and torch.equal(got.probs[m], before[3][m]), (m, kw)
            else:                                      # dg_sample_rows_control bit for bit; the only addition is the budget write
                assert torch.equal(got.ids[m], ref.ids[m]) and torch.equal(got.cbuf[m], ref.cbuf[m]), (m, kw)
                assert torch.equal(got.probs[m], ref.probs[m]), (m, kw)
                tok = int(got.ids[m, L])
                assert 0 <= tok < Vx and not np.isneginf(bias[tok]) and float(got.probs[m, tok]) > 0
                assert int(got.cbuf[m, tok]) == counts[m, tok] + 1
                assert torch.equal(got.ids[m, :L], ids[m, :L].to(dev)) and torch.equal(got.ids[m, L + 1:], ids[m, L + 1:].to(dev))
                end = SPANS[r][0][1]
                want_len = int(ref.lengths[m]) or (L + 1 if L + 1 >= end else 0)
                assert int(got.lengths[m]) == want_len, (m, r, kw)
                if r == "stop":
                    assert tok in stop and want_len == L + 1 == int(ref.lengths[m])
                if r == "budget":
                    assert int(got.lengths[m]) == L + 1
                    if n == 0:
                        assert tok not in stop and int(ref.lengths[m]) == 0            # ended by its budget, not by a stop token
                if r == "sample" and tok not in stop:
                    assert int(got.lengths[m]) == 0
        assert (got.cbuf[:, Vx:] == 12345).all() and (got.probs[:, Vx:] == 7.0).all()
        assert torch.isfinite(got.probs[live, :Vx]).all()


@pytest.mark.parametrize("Vx,M", [(80, 8), (50257, 4)])
def test_all_rows_forced_nothing_changes(dev, Vx, M):
    from drakegpt_amd import ops
    x, counts, bias, ids = kernel_inputs(Vx, M, 7)
    got = Operands(dev, np.full_like(x, np.nan), counts, bias, [0] * M, ids)
    before = got.snapshot()
    spans = torch.tensor([[L + 1 + m, L + 20] for m in range(M)], dtype=torch.int32, device=dev)
    ctl = ops.new_sample_control(repetition_penalty=1.3, stop_tokens=(3,), use_bias=True, device=dev)
    for params in (ops.new_sample_params(1.0, None, dev, four=True), ops.new_sample_params(0.0, 5, dev, top_p=0.5, four=True)):
        assert got.launch("dg_sample_rows_ragged", params, ctl, spans) == 0
        assert all(torch.equal(a, b) for a, b in zip(got.snapshot(), before))
    # through the wrapper too, which needs control, lengths and the 2-D ids
    ops.sample_rows(got.logits, got.state, ids=got.ids, control=ctl, counts=got.counts, lengths=got.lengths, spans=spans)
    assert all(torch.equal(a, b) for a, b in zip(got.snapshot(), before))
    with pytest.raises(ValueError):
        ops.sample_rows(got.logits, got.state, ids=got.ids, control=ctl, counts=got.counts, spans=spans)
    with pytest.raises(ValueError):
        ops.sample_rows(got.logits, got.state, ids=got.ids, spans=spans)
    with pytest.raises(ValueError):
        ops.sample_rows(got.logits, seed=5, L=L, control=ctl, lengths=got.lengths, spans=spans)
    with pytest.raises(RuntimeError):
        ops.sample_rows(got.logits, got.state, ids=got.ids, control=ctl, lengths=got.lengths, spans=spans[:, :1].contiguous())


def test_refusals_return_the_argument_error_and_launch_nothing(dev):
    from drakegpt_amd import ops
    Vx, M = 80, 4
    x, counts, bias, ids = kernel_inputs(Vx, M, 9)
    got = Operands(dev, x, counts, bias, [0] * M, ids)
    before = got.snapshot()
    spans = torch.tensor([[1, 20]] * M, dtype=torch.int32, device=dev)
    ctl = ops.new_sample_control(device=dev)
    params = ops.new_sample_params(1.0, None, dev, four=True)
    assert got.launch("dg_sample_rows_ragged", params, ctl, None) == ERR_ARG                     # NULL spans
    assert got.launch("dg_sample_rows_ragged", params, ctl, spans, lengths=None) == ERR_ARG
    assert got.launch("dg_sample_rows_ragged", params, ctl, spans, ids=None) == ERR_ARG
    assert got.launch("dg_sample_rows_ragged", params, ctl, spans, ld_ids=0) == ERR_ARG
    # ... and whatever the control entry refuses
    assert got.launch("dg_sample_rows_ragged", params, None, spans) == ERR_ARG                   # NULL control
    assert got.launch("dg_sample_rows_ragged", None, ctl, spans) == ERR_ARG                      # NULL params
    assert got.launch("dg_sample_rows_ragged", params, ctl, spans, state=None) == ERR_ARG        # ids without a state
    assert got.launch("dg_sample_rows_ragged", params, ctl, spans, logits=None) == ERR_ARG
    assert got.launch("dg_sample_rows_ragged", params, ctl, spans, ld_ids=-1) == ERR_ARG
    assert all(torch.equal(a, b) for a, b in zip(got.snapshot(), before))
    assert got.launch("dg_sample_rows_ragged", params, ctl, spans) == 0                          # the same operands, complete
    assert not torch.equal(got.ids, before[0])


@pytest.mark.parametrize("Vx", [80, 50257])
def test_token_counts_per_row_equals_bincount(dev, Vx):
    from drakegpt_amd import ops
    M, cap = 6, 320
    g = np.random.default_rng(Vx)
    ids = g.integers(0, Vx, size=(M, cap))
    ids[0, 0], ids[1, 0], ids[2, 299] = -3, Vx + 10, 2 ** 40                # clamped as the embedding clamps
    n = [1, 5, 300, 300, 1, 5]
    idd = torch.from_numpy(ids).to(dev)
    want = np.stack([CM.count_prefix(ids[m:m + 1, :n[m]], Vx)[0] for m in range(M)])
    spans = torch.tensor([[q, q + 9] for q in n], dtype=torch.int32, device=dev)
    buf = torch.full((M, Vx + 3), 99, dtype=torch.int32, device=dev)
    c = ops.token_counts(idd, spans[:, 0], Vx, buf[:, :Vx])                 # the spans' first column: stride 2; zeroing, ldc > V
    assert (c.cpu().numpy() == want).all() and (buf[:, Vx:] == 99).all()
    ops.token_counts(idd, torch.tensor(n, dtype=torch.int32, device=dev), Vx, c, accumulate=True)          # stride 1, accumulating
    assert (c.cpu().numpy() == 2 * want).all() and (buf[:, Vx:] == 99).all()
    assert (ops.token_counts(idd, spans[:, 0], Vx).cpu().numpy() == want).all()
    # n is clamped to [0, capacity]
    wild = torch.tensor([-4, 0, cap, cap + 1000, 2 ** 31 - 1, 1], dtype=torch.int32, device=dev)
    want = np.stack([CM.count_prefix(ids[m:m + 1, :q], Vx)[0] for m, q in enumerate([0, 0, cap, cap, cap, 1])])
    assert (ops.token_counts(idd, wild, Vx).cpu().numpy() == want).all()
    with pytest.raises(RuntimeError):
        ops.token_counts(idd, spans[:4, 0], Vx)
    with pytest.raises(TypeError):
        ops.token_counts(idd, spans[:, 0].long(), Vx)
    with pytest.raises(RuntimeError):
        ops.token_counts(idd[:, :100], spans[:, 0], Vx)                     # not whole rows: the clamp would not be the capacity


# ------------------------------------------------------------------------------------------------------------------ end to end
PROMPTS = [[2, 3], [5, 7, 1, 4, 9, 11, 13, 2, 6], [1, 4, 8, 3, 10]]          # lengths 2, 9, 5
PEN = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={11: NINF, 20: 1.5}, top_k=30, top_p=0.95)


def batch(dev, prompts, fill=0, width=None):
    idx, p = RM.pad_prompts(prompts, fill, width)
    return torch.from_numpy(idx).to(dev), p


def long_prompts(lengths):
    return [[(7 * j + 3 * b + 2) % 78 for j in range(n)] for b, n in enumerate(lengths)]


def ragged(m, idx, p, n_new, seed=11, **kw):
    kw.setdefault("pad_token", PAD)
    return m.generate(idx, n_new, sampler="device", seed=seed, prompt_lengths=p, return_lengths=True, **kw)


def eager(m, idx, p, n_new, seed=11, **kw):
    """the graph-replayed path's steps launched one by one (graph=False), from generate()'s own checks"""
    import inspect
    from drakegpt_amd.model import Sampling
    sig = inspect.signature(m.generate).parameters
    names = ["temperature", "top_k", "seed", "top_p", "min_p", "repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias",
             "stop_tokens", "pad_token", "stop_poll"]
    kw = dict(kw, seed=seed)
    kw.setdefault("pad_token", PAD)
    req = Sampling.checked(V, None, "device", *[kw.get(k, sig[k].default) for k in names], p, tuple(idx.shape), True)
    idx, done = req.enter(idx, n_new)
    assert done is None
    return m._generate_device_cached(idx, n_new, req, graph=False)


def rows_of_rectangular_runs(m, prompts, n_new, seed=11, **kw):
    """per prompt b: (row b, its final length) of the call on prompt b repeated B times -- no prompt_lengths anywhere"""
    dev = next(m.parameters()).device
    out = []
    for b, r in enumerate(prompts):
        ids, n = m.generate(torch.tensor([r] * len(prompts), device=dev), n_new, sampler="device", seed=seed, return_lengths=True, **kw)
        out.append((ids[b].tolist(), int(n[b])))
    return out


def check_rows(out, lens, prompts, want, n_new, pad=PAD):
    out, lens = out.cpu().tolist(), lens.tolist()
    assert len(out[0]) == max(lens)
    for b, (r, (ref, end)) in enumerate(zip(prompts, want)):
        assert lens[b] == end <= len(r) + n_new, (b, lens, end)
        assert out[b][:len(r)] == r, b                                     # the prompt is preserved
        assert out[b][:end] == ref[:end], (b, out[b], ref)
        assert all(t == pad for t in out[b][end:]), b


def test_fp32_rows_equal_rectangular_runs(dev):
    m = lm(dev)
    idx, p = batch(dev, PROMPTS, fill=V + 1000)                            # what lies in the padding never reaches a kernel
    out, lens = ragged(m, idx, p, NEW)                                     # every row crosses the window at 32
    assert out.shape == (3, 9 + NEW) and lens.dtype == torch.int64 and lens.device == out.device
    assert lens.tolist() == [q + NEW for q in p]
    check_rows(out, lens, PROMPTS, rows_of_rectangular_runs(m, PROMPTS, NEW), NEW)
    assert idx[0, 2] == V + 1000                                           # the caller's tensor is as it was
    # the default return is the ids alone; a wider idx changes nothing
    wide, _ = batch(dev, PROMPTS, fill=-7, width=14)
    assert torch.equal(m.generate(wide, NEW, sampler="device", seed=11, prompt_lengths=torch.tensor(p), pad_token=PAD), out)
    # no new tokens: the padded prompts
    o0, l0 = ragged(m, idx, p, 0)
    assert o0.tolist() == RM.pad_prompts(PROMPTS, PAD)[0].tolist() and l0.tolist() == p
    # return_lengths on a rectangular call
    o1, l1 = m.generate(idx[:, :2].contiguous(), 5, sampler="device", seed=11, return_lengths=True)
    assert o1.shape == (3, 7) and l1.tolist() == [7, 7, 7] and l1.dtype == torch.int64


@pytest.mark.parametrize("lengths,n_new", [((3, 40), 6), ((32, 35), 6), ((33, 36), 4), ((1, 6), 34), ((31, 32, 33), 5)],
                         ids=["past_window", "t_min_is_ctx", "no_prefill", "t_min_1", "around_ctx"])
def test_window_and_prefill_edges_and_path_equality_fp32(dev, lengths, n_new):
    """forced steps in both graphs (a prompt longer than the window), t_min >= ctx (no prefill), t_min == 1; graph == eager ==
    uncached == the rows of the rectangular uncached runs"""
    m = lm(dev)
    prompts = long_prompts(lengths)
    idx, p = batch(dev, prompts, fill=5)
    out, lens = ragged(m, idx, p, n_new)
    assert lens.tolist() == [q + n_new for q in p] and out.shape == (len(p), max(p) + n_new)
    e_out, e_lens = eager(m, idx, p, n_new)
    assert out.tolist() == e_out.tolist() and lens.tolist() == e_lens.tolist()
    u_out, u_lens = ragged(m, idx, p, n_new, use_cache=False)
    assert out.tolist() == u_out.tolist() and lens.tolist() == u_lens.tolist()
    check_rows(out, lens, prompts, rows_of_rectangular_runs(m, prompts, n_new, use_cache=False), n_new)


def test_bf16_graph_equals_eager_and_the_structure_holds(dev):
    m = lm(dev, "bf16")
    idx, p = batch(dev, PROMPTS)
    out, lens = ragged(m, idx, p, NEW, logit_bias={PAD: NINF})             # the pad token is never drawn: the structure is exact
    e_out, e_lens = eager(m, idx, p, NEW, logit_bias={PAD: NINF})
    assert out.tolist() == e_out.tolist() and lens.tolist() == e_lens.tolist() == [q + NEW for q in p]
    for b, r in enumerate(PROMPTS):
        row = out[b].tolist()
        assert row[:len(r)] == r and PAD not in row[len(r):len(r) + NEW] and all(t == PAD for t in row[len(r) + NEW:])
        assert all(0 <= t < V for t in row)


def test_controls_stop_tokens_and_the_poll(dev):
    m = lm(dev)
    idx, p = batch(dev, PROMPTS)
    plain, lens = ragged(m, idx, p, NEW, **PEN)
    assert lens.tolist() == [q + NEW for q in p]
    check_rows(plain, lens, PROMPTS, rows_of_rectangular_runs(m, PROMPTS, NEW, **PEN), NEW)
    assert all(11 not in plain[b, q:].tolist() for b, q in enumerate(p))
    # stop tokens from the run itself: rows 0 and 1 end early
    gen = [plain[b, q:q + NEW].tolist() for b, q in enumerate(p)]
    stop = (gen[0][12], next(t for t in gen[1][20:30] if t != gen[0][12]))
    outs = [ragged(m, idx, p, NEW, stop_tokens=stop, stop_poll=poll, **PEN) for poll in (1, 64)]
    out, lens = outs[0]
    assert out.tolist() == outs[1][0].tolist() and lens.tolist() == outs[1][1].tolist()              # the poll changes nothing
    assert lens[0] <= p[0] + 13 and lens[1] <= p[1] + 30                   # stopped rows end at the stop, not at their budget
    for b, q in enumerate(p):
        end = int(lens[b])
        assert out[b, :end].tolist() == plain[b, :end].tolist() and (out[b, end:] == PAD).all()
        assert end == q + NEW or int(out[b, end - 1]) in stop
        assert not set(out[b, q:end - 1].tolist()) & set(stop)
    check_rows(out, lens, PROMPTS, rows_of_rectangular_runs(m, PROMPTS, NEW, stop_tokens=stop, pad_token=PAD, **PEN), NEW)
    e_out, e_lens = eager(m, idx, p, NEW, stop_tokens=stop, stop_poll=7, **PEN)
    assert out.tolist() == e_out.tolist() and lens.tolist() == e_lens.tolist()
    u_out, u_lens = ragged(m, idx, p, NEW, stop_tokens=stop, stop_poll=7, use_cache=False, **PEN)
    assert out.tolist() == u_out.tolist() and lens.tolist() == u_lens.tolist()
    # every row stops: the result is trimmed to the longest of them; the default pad is the first stop token
    stop += (next(t for t in gen[2][:30] if t not in stop),)
    out, lens = ragged(m, idx, p, NEW, stop_tokens=stop, pad_token=None, **PEN)
    assert out.shape[1] == int(lens.max()) < max(p) + NEW
    assert all((out[b, int(lens[b]):] == stop[0]).all() for b in range(3))


@pytest.mark.parametrize("use_cache", [True, False])
def test_equal_lengths_are_the_call_without_prompt_lengths(dev, use_cache):
    m = lm(dev)
    idx = torch.tensor(long_prompts((5, 5, 5)), device=dev)
    for kw in (dict(), dict(temperature=0.8, top_k=20), PEN):
        want = m.generate(idx, NEW, sampler="device", seed=3, use_cache=use_cache, **kw)
        got, lens = m.generate(idx, NEW, sampler="device", seed=3, use_cache=use_cache, prompt_lengths=[5, 5, 5], pad_token=PAD,
                               return_lengths=True, **kw)
        assert got.tolist() == want.tolist() and lens.tolist() == [5 + NEW] * 3
        want = m.generate(idx, 12, torch.Generator().manual_seed(3), use_cache=use_cache, **kw)
        got = m.generate(idx, 12, torch.Generator().manual_seed(3), use_cache=use_cache, prompt_lengths=(5, 5, 5), pad_token=PAD, **kw)
        assert got.tolist() == want.tolist()


def test_one_decoder_three_graph_pairs(dev):
    m = lm(dev)
    idx, p = batch(dev, PROMPTS)
    first = m.generate(idx[:, :2].contiguous(), NEW, sampler="device", seed=11)
    (dec,) = m._decoders.values()
    plain_pair = dec.graphs
    assert plain_pair is not None and dec.graphs_control is None and dec.graphs_ragged is None
    ctl = m.generate(idx[:, :2].contiguous(), NEW, sampler="device", seed=11, repetition_penalty=1.3)
    control_pair = dec.graphs_control
    assert control_pair is not None and dec.graphs_ragged is None and dec.graphs is plain_pair
    r1, l1 = ragged(m, idx, p, NEW)
    ragged_pair = dec.graphs_ragged
    assert ragged_pair is not None and dec.graphs is plain_pair and dec.graphs_control is control_pair
    again = m.generate(idx[:, :2].contiguous(), NEW, sampler="device", seed=11)
    assert torch.equal(again, first)                                       # bit for bit, after both other pairs ran
    assert torch.equal(m.generate(idx[:, :2].contiguous(), NEW, sampler="device", seed=11, repetition_penalty=1.3), ctl)
    # other lengths and settings: no new capture, no new decoder, and nothing inherited -- not even from poisoned operands
    dec.counts.fill_(1000)
    dec.lengths.fill_(1)
    dec.spans.fill_(10 ** 6)
    other = [PROMPTS[1], PROMPTS[2][:3], PROMPTS[0] + [9, 9]]
    idx2, p2 = batch(dev, other)
    kw = dict(temperature=0.9, top_p=0.9, frequency_penalty=0.3, stop_tokens=int(r1[0, 20]))
    r2, l2 = ragged(m, idx2, p2, 30, seed=4, **kw)
    assert list(m._decoders.values()) == [dec]
    assert dec.graphs is plain_pair and dec.graphs_control is control_pair and dec.graphs_ragged is ragged_pair
    f2, fl2 = ragged(lm(dev), idx2, p2, 30, seed=4, **kw)
    assert r2.tolist() == f2.tolist() and l2.tolist() == fl2.tolist()
    r3, l3 = ragged(m, idx, p, NEW)
    assert r3.tolist() == r1.tolist() and l3.tolist() == l1.tolist()


@pytest.mark.parametrize("use_cache", [True, False])
def test_host_sampler(dev, use_cache):
    m = lm(dev)
    idx, p = batch(dev, PROMPTS, fill=V + 5)                               # out-of-range ids in the pad columns are accepted
    n_new = 30                                                             # 9 + 30 tokens: crosses the window
    kw = dict(use_cache=use_cache, prompt_lengths=p, pad_token=PAD, logit_bias={PAD: NINF}, return_lengths=True)
    out, lens = m.generate(idx, n_new, torch.Generator().manual_seed(3), **kw)
    assert out.shape == (3, 9 + n_new) and lens.tolist() == [q + n_new for q in p] and lens.device == out.device
    for b, r in enumerate(PROMPTS):
        row = out[b].tolist()
        assert row[:len(r)] == r                                           # prompts preserved
        assert PAD not in row[len(r):len(r) + n_new] and all(0 <= t < V for t in row)      # exactly n_new tokens ...
        assert all(t == PAD for t in row[len(r) + n_new:])                 # ... then pads
    again, _ = m.generate(idx, n_new, torch.Generator().manual_seed(3), **kw)
    assert again.tolist() == out.tolist()
    assert m.generate(idx, n_new, torch.Generator().manual_seed(4), **kw)[0].tolist() != out.tolist()
    # greedy with a penalty: both samplers agree, so the forced tokens are counted once and the budget ends each row
    g = dict(temperature=0.0, frequency_penalty=0.7, prompt_lengths=p, pad_token=PAD, return_lengths=True)
    h_out, h_lens = m.generate(idx, n_new, torch.Generator().manual_seed(1), use_cache=use_cache, **g)
    d_out, d_lens = m.generate(idx, n_new, sampler="device", seed=1, use_cache=use_cache, **g)
    assert h_out.tolist() == d_out.tolist() and h_lens.tolist() == d_lens.tolist()
    # a stop token ends a row before its budget; a stop token inside a prompt ends nothing
    stop = int(h_out[1, p[1] + 10])
    s_out, s_lens = m.generate(idx, n_new, torch.Generator().manual_seed(1), use_cache=use_cache, stop_tokens=list({stop: 0, PROMPTS[1][2]: 0}), **g)
    assert p[1] < int(s_lens[1]) <= p[1] + 11 and s_out[1, :int(s_lens[1])].tolist() == h_out[1, :int(s_lens[1])].tolist()
    assert (s_out[1, int(s_lens[1]):] == PAD).all() and s_out.shape[1] == int(s_lens.max())


def test_bigram_smoke_both_samplers(dev):
    import drakegpt_amd as D
    torch.manual_seed(0)
    m = D.BigramLM(V).to(dev).eval()
    idx, p = batch(dev, PROMPTS, fill=-1)
    kw = dict(prompt_lengths=p, pad_token=PAD, logit_bias={PAD: NINF}, return_lengths=True)
    for out, lens in (m.generate(idx, 20, sampler="device", seed=3, **kw), m.generate(idx, 20, torch.Generator().manual_seed(1), **kw)):
        assert out.shape == (3, 29) and lens.tolist() == [q + 20 for q in p]
        for b, r in enumerate(PROMPTS):
            row = out[b].tolist()
            assert row[:len(r)] == r and PAD not in row[len(r):len(r) + 20] and all(t == PAD for t in row[len(r) + 20:])
    d = rows_of_rectangular_runs(m, PROMPTS, 20, seed=3, logit_bias={PAD: NINF})
    out, lens = m.generate(idx, 20, sampler="device", seed=3, **kw)
    check_rows(out, lens, PROMPTS, d, 20)
