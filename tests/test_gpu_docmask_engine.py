"""Document-masked attention above the kernels: set_doc_separator on the models, TrainEngine(doc_separator=), the harness flag.

Configuration: V 80, C 128, two heads of 64, 2 layers, T 64, B 4 (fp32 and bf16; fp8 at C 256, four heads, so that the fp8 GEMMs
take the contractions), and the scaled preset at B 16 for the block-chain forward.  The model is held to a torch fp64 restatement
of the blocks with the mask start[i] <= j <= i at the model-level tolerances the suite uses per precision (fp32 1e-4; bf16 logits
3e-2, loss 2e-2; fp8 logits 5e-2), the engine to autograd through the module path, the captured step to the eager one bit for
bit.  The kernels themselves: tests/test_gpu_docmask.py."""
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import docmask_cases as D  # noqa: E402

pytestmark = pytest.mark.gpu

V, T, B, L = 80, 64, 4, 2
SEP = 7
CFG = {"fp32": (128, 2), "bf16": (128, 2), "fp8": (256, 4)}          # precision -> (C, heads of 64)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _model(dev, precision, p=0.0, seed=42):
    import drakegpt_amd as DG
    C, NH = CFG[precision]
    torch.manual_seed(seed)
    return DG.TransformerLM(V, C, T, NH, L, p, precision=precision).to(dev)


def _batch(seed=0, n_sep=3, rows=B):
    """ids without the separator, then n_sep separators per row at positions of the row's own (one row with none at all, one
    with a separator at position 0 and at T - 1)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, V - 1, (rows, T), generator=g)
    x[x == SEP] = V - 1
    for b in range(1, rows):
        x[b, torch.randperm(T, generator=g)[:n_sep]] = SEP
    if rows > 2:
        x[2, 0] = SEP
        x[2, T - 1] = SEP
    y = torch.randint(0, V, (rows, T), generator=g)
    return x, y


def _starts(x):
    s = torch.zeros_like(x)
    for b in range(x.shape[0]):
        a = 0
        for t in range(x.shape[1]):
            s[b, t] = a
            if x[b, t] == SEP:
                a = t + 1
    return s


def _restatement(sd, x, y, NH):
    """TransformerLM.forward in fp64 with the document mask (dropout off): logits [B, T, V], loss"""
    sd = {k: v.detach().double().cpu() for k, v in sd.items()}
    Bn, Tn = x.shape
    s = _starts(x)
    j = torch.arange(Tn)
    mask = (j.view(1, 1, Tn) <= j.view(1, Tn, 1)) & (j.view(1, 1, Tn) >= s.view(Bn, Tn, 1))          # [B, T, T]
    h = sd["token_embedding_table.weight"][x] + sd["position_embedding_table.weight"][:Tn]
    ln = torch.nn.functional.layer_norm
    for l in range(L):
        pre = f"blocks.{l}."
        a = ln(h, h.shape[-1:], sd[pre + "ln1.weight"], sd[pre + "ln1.bias"])
        outs = []
        for hd in range(NH):
            q, k, v = (a @ sd[f"{pre}sa_head.heads.{hd}.{n}.weight"].T for n in ("query", "key", "value"))
            w = (q @ k.transpose(-2, -1) * q.shape[-1] ** -0.5).masked_fill(~mask, float("-inf")).softmax(-1)
            outs.append(w @ v)
        h = h + torch.cat(outs, -1) @ sd[pre + "sa_head.proj.weight"].T + sd[pre + "sa_head.proj.bias"]
        a = ln(h, h.shape[-1:], sd[pre + "ln2.weight"], sd[pre + "ln2.bias"])
        f = torch.relu(a @ sd[pre + "ffwd.net.0.weight"].T + sd[pre + "ffwd.net.0.bias"])
        h = h + f @ sd[pre + "ffwd.net.2.weight"].T + sd[pre + "ffwd.net.2.bias"]
    logits = h @ sd["lm_head.weight"].T + sd["lm_head.bias"]
    return logits, torch.nn.functional.cross_entropy(logits.view(-1, V), y.view(-1))


@pytest.mark.parametrize("precision,tol_logits,tol_loss", [("fp32", 1e-4, 1e-4), ("bf16", 3e-2, 2e-2), ("fp8", 5e-2, 2e-2)])
def test_model_matches_the_masked_restatement(dev, precision, tol_logits, tol_loss):
    """forward(idx, targets) with a separator set, in eval() and in train() (dropout 0), against the fp64 restatement; without
    the separator the same model differs from it (the mask is what is being compared)"""
    m = _model(dev, precision).eval()
    x, y = _batch()
    ref_logits, ref_loss = _restatement(m.state_dict(), x, y, CFG[precision][1])
    plain = m(x.to(dev), y.to(dev))[0]
    assert m.set_doc_separator(SEP) is m and m.doc_separator == SEP
    for mode in ("eval", "train"):
        getattr(m, mode)()
        logits, loss = m(x.to(dev), y.to(dev))
        e = rel(logits.view(B, T, V), ref_logits)
        print(f"docmask model {precision} {mode}: logits {e:.3e} (bound {tol_logits:g}), loss {abs(loss.item() - ref_loss.item()) / ref_loss.item():.3e}")
        assert e < tol_logits, e
        assert abs(loss.item() - ref_loss.item()) < tol_loss * ref_loss.item()
    if precision == "fp32":
        assert rel(plain.view(B, T, V)[1:], ref_logits[1:]) > 1e-3             # (the unmasked model is far outside the bound)
    assert rel(plain.view(B, T, V)[0], ref_logits[0]) < tol_logits          # (row 0 holds no separator)
    m.set_doc_separator(None)
    assert torch.equal(m.eval()(x.to(dev), y.to(dev))[0], plain)
    for bad in (-1, V, 1.5, True):
        with pytest.raises(ValueError):
            m.set_doc_separator(bad)


def test_every_model_takes_the_option(dev):
    import drakegpt_amd as DG
    x = _batch()[0][:, :8].contiguous().to(dev)
    kw = dict(BigramLM=dict(vocab_size=V), SingleHeadAttentionLM=dict(vocab_size=V, embedding_dim=32, context_length=8, head_size=32),
              MultiHeadAttentionLM=dict(vocab_size=V, embedding_dim=32, context_length=8, head_size=32, num_heads=4),
              BlocksLM=dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=2),
              ResidualBlocksLM=dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=2),
              TransformerLM=dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=2, dropout=0.0))
    x[:, 3] = SEP
    other = x.clone()
    other[:, :3] = (other[:, :3] + 1) % (V - 1)
    other[:, :3][other[:, :3] == SEP] = V - 1
    for name, k in kw.items():
        torch.manual_seed(1)
        m = DG.MODEL_CLASSES[name](**k).to(dev).eval()
        assert m.set_doc_separator(SEP) is m
        a, b = m(x)[0], m(other)[0]
        assert torch.equal(a[:, 4:], b[:, 4:]), name                         # nothing before the separator reaches behind it
        if name != "BigramLM":
            m.set_doc_separator(None)
            assert not torch.equal(m(x)[0][:, 4:], m(other)[0][:, 4:]), name


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_tokens_before_a_separator_do_not_reach_behind_it(dev, precision):
    """changing the tokens before a separator leaves the logits behind it bit for bit, in eval() and in train() with dropout
    (keyed by position and step, so the same in both runs)"""
    x, _ = _batch(rows=2, n_sep=0)
    cut = 30
    x[:, cut] = SEP
    other = x.clone()
    other[:, :cut] = (other[:, :cut] + 5) % (V - 1)
    other[:, :cut][other[:, :cut] == SEP] = V - 1
    for mode, p in (("eval", 0.0), ("train", 0.2)):
        res = []
        for ids in (x, other):
            m = _model(dev, precision, p=p).set_doc_separator(SEP)
            getattr(m, mode)()
            res.append(m(ids.to(dev))[0])
        assert bool(torch.isfinite(res[0]).all())
        assert torch.equal(res[0][:, cut + 1:], res[1][:, cut + 1:]), mode
        assert not torch.equal(res[0][:, :cut], res[1][:, :cut])


def _corpus(n=6000, every=23, seed=1):
    c = torch.randint(0, V - 1, (n,), generator=torch.Generator().manual_seed(seed))
    c[c == SEP] = V - 1
    c[torch.randint(0, n, (n // every,), generator=torch.Generator().manual_seed(seed + 1))] = SEP
    return c


def _engine(dev, precision, graph, p=0.0, corpus=None, rows=None, **kw):
    from drakegpt_amd.engine import TrainEngine
    m = _model(dev, precision, p=p).train()
    eng = TrainEngine(m, B, T, lr=1e-3, betas=(0.9, 0.95), seed=11, use_graph=graph, **kw)
    if corpus is not None:
        eng.set_corpus(corpus.to(dev))
        eng.stage_offsets(rows)
    return m, eng


def _grads(eng):
    return {k: v.detach().clone().cpu() for k, v in eng.named_grads().items()}


def _same_grads(a, b, exact_tok):
    for k in a:
        if k == "token_embedding_table.weight" and not exact_tok:          # (fp32 atomics in a free order without the one-hot GEMM)
            assert torch.allclose(a[k], b[k], rtol=1e-5, atol=1e-9)
        else:
            assert torch.equal(a[k], b[k]), k


def test_engine_step_equals_autograd_through_the_module_path(dev):
    """fp32, two consecutive steps on staged offsets with doc_separator: each step's loss and flat gradient equal autograd through
    the module path with set_doc_separator at the weights the step started from (loss 1e-5, flat gradient 1e-4: the suite's fp32
    bounds for the two paths)"""
    corpus = _corpus()
    rows = torch.randint(0, 6000 - T - 1, (2, B), generator=torch.Generator().manual_seed(5))
    m, eng = _engine(dev, "fp32", True, corpus=corpus, rows=rows, doc_separator=SEP)
    assert eng.doc_separator == SEP and eng.doc_starts.dtype == torch.int32 and eng.doc_starts.numel() == B * T
    for r in rows:
        x = torch.stack([corpus[o:o + T] for o in r.tolist()]).to(dev)
        y = torch.stack([corpus[o + 1:o + T + 1] for o in r.tolist()]).to(dev)
        assert int((x == SEP).sum()) > 0
        m2 = _model(dev, "fp32", seed=3).train().set_doc_separator(SEP)
        m2.load_state_dict({k: v.detach().clone() for k, v in m.state_dict().items()})
        _, loss2 = m2(x, y)
        loss2.backward()
        want = {k: p.grad for k, p in m2.named_parameters() if p.grad is not None}
        loss = eng.step().item()
        torch.cuda.synchronize()
        assert torch.equal(eng.doc_starts.cpu().view(B, T).long(), _starts(x.cpu()))
        got = eng.named_grads()
        keys = [k for k in got if k in want]
        assert len(keys) >= len(got) - 2                                      # (ln_f has no gradient)
        assert abs(loss - loss2.item()) < 1e-5 * abs(loss2.item()), (loss, loss2.item())
        e = rel(torch.cat([got[k].reshape(-1) for k in keys]), torch.cat([want[k].reshape(-1) for k in keys]))
        assert e < 1e-4, e
        # and the mask matters: the default module path disagrees on this batch
        m2.set_doc_separator(None)
        assert abs(m2(x, y)[1].item() - loss) > 2e-5 * loss


@pytest.mark.parametrize("config", ["fp32", "bf16", "fp8", "scaled-chain"])
def test_captured_step_equals_eager_and_reads_fresh_starts(dev, config):
    """three steps with dropout on staged offsets, captured against eager.  The first step: the same loss and the same gradient bit
    for bit (fp8: the loss; the token table, where it is an fp32 scatter-add with atomics in a free order, to 1e-5 as everywhere
    in the suite).  The later steps bit for bit where the whole step is free of atomics (bf16 with the one-hot dW problem, the
    chain configuration); in fp32 the weights behind the first AdamW step differ by that scatter-add's order and the losses are
    held to 2e-6, the criterion of test_graph_equals_eager_with_dropout; in fp8 to the suite's fp8 loss bound 1e-3.  Why fp8
    differs from the third step on, with or without the option: the seeding step fills all three slots of an attention site's amax
    history with its maximum a0 and runs no fp8 attention kernel, so nothing clears slot 1; the eager second step then collects
    its maxima on top of a0 and the third step scales with max(a0, a1), while the captured program replays step 0 behind its
    warm-up, which clears slot 1, and its third step scales with a1 alone -- different bits whenever a1 < a0 at any site.  The
    replays read the starts of their own batch: the buffer after each step is that batch's, and differs from the one before."""
    import drakegpt_amd as DG
    from drakegpt_amd.engine import TrainEngine
    corpus = _corpus(20_000)
    res = []
    for graph in (False, True):
        if config == "scaled-chain":
            Bs, Ts = 16, 256
            torch.manual_seed(42)
            m = DG.TransformerLM(V, 384, Ts, 6, 2, 0.2, precision="bf16").to(dev).train()
            eng = TrainEngine(m, Bs, Ts, lr=3e-4, betas=(0.9, 0.95), seed=7, use_graph=graph, doc_separator=SEP)
            assert eng.chain_full
            eng.set_corpus(corpus.to(dev))
            rows = torch.randint(0, 20_000 - Ts - 1, (3, Bs), generator=torch.Generator().manual_seed(2))
            eng.stage_offsets(rows)
        else:
            Bs, Ts = B, T
            rows = torch.randint(0, 20_000 - T - 1, (3, B), generator=torch.Generator().manual_seed(2))
            m, eng = _engine(dev, config, graph, p=0.1, corpus=corpus, rows=rows, doc_separator=SEP)
            assert eng.fp8 == (config == "fp8")
        losses, starts, first = [], [], None
        for r in rows:
            losses.append(eng.step().item())
            torch.cuda.synchronize()
            first = _grads(eng) if first is None else first
            x = torch.stack([corpus[o:o + Ts] for o in r.tolist()])
            assert torch.equal(eng.doc_starts.cpu().view(Bs, Ts).long(), _starts(x))
            starts.append(eng.doc_starts.clone())
        assert all(math.isfinite(v) for v in losses)
        assert not torch.equal(starts[0], starts[1]) and not torch.equal(starts[1], starts[2])
        if graph:
            assert len(eng._graphs) == 1                                       # one graph launch per step, as without the option
        res.append((losses, _grads(eng), eng.onehot is not None, first))
    (la, ga, exact, fa), (lb, gb, _, fb) = res
    print(f"docmask captured vs eager {config}: losses {la} / {lb}")
    assert la[0] == lb[0], (la, lb)
    if config != "fp8":
        _same_grads(fa, fb, exact_tok=exact)
    if exact and config != "fp8":
        assert la == lb, (la, lb)
        _same_grads(ga, gb, exact_tok=True)
    else:
        tol = 1e-3 if config == "fp8" else 2e-6
        assert all(abs(a - b) <= tol * abs(b) for a, b in zip(la, lb)), (la, lb)


@pytest.mark.parametrize("config", ["fp32", "scaled-chain"])
def test_step_launches_are_the_default_engines_plus_one(dev, config):
    """the eager step's library calls: the default engine's, with dg_doc_starts right behind the embedding launch and the two
    attention entries replaced by their document forms -- one call more, nothing else moved"""
    import drakegpt_amd as DG
    from drakegpt_amd import ops
    from drakegpt_amd.engine import TrainEngine
    corpus = _corpus(20_000)
    traces = []
    for kw in ({}, {"doc_separator": SEP}):
        if config == "scaled-chain":
            torch.manual_seed(42)
            m = DG.TransformerLM(V, 384, 256, 6, 2, 0.2, precision="bf16").to(dev).train()
            eng = TrainEngine(m, 16, 256, lr=3e-4, betas=(0.9, 0.95), seed=7, use_graph=False, **kw)
            eng.set_corpus(corpus.to(dev))
            eng.stage_offsets(torch.randint(0, 20_000 - 257, (2, 16), generator=torch.Generator().manual_seed(2)))
        else:
            _, eng = _engine(dev, config, False, corpus=corpus, rows=torch.randint(0, 20_000 - T - 1, (2, B), generator=torch.Generator().manual_seed(2)), **kw)
        calls = []
        check = ops.check

        def counting(rc, what):
            calls.append(what)
            return check(rc, what)
        ops.check = counting
        try:
            eng.step()
        finally:
            ops.check = check
        torch.cuda.synchronize()
        traces.append(calls)
    plain, doc = traces
    assert "dg_doc_starts" not in plain and not any(c.endswith("_doc") for c in plain)
    assert len(doc) == len(plain) + 1
    i = doc.index("dg_doc_starts")
    assert doc.count("dg_doc_starts") == 1 and "embed" in doc[i - 1]
    rest = doc[:i] + doc[i + 1:]
    back = {"dg_attn_fwd_doc": ("dg_attn_fwd", "dg_attn_fwd_fp8"), "dg_attn_bwd_doc": ("dg_attn_bwd", "dg_attn_bwd_fp8")}
    assert all(a == b or b in back.get(a, ()) for a, b in zip(rest, plain)), [(a, b) for a, b in zip(rest, plain) if a != b][:4]
    assert rest.count("dg_attn_fwd_doc") == 2 and rest.count("dg_attn_bwd_doc") == 2


def test_a_batch_without_the_separator_is_the_default_step(dev):
    """fp32: with no separator in the batch the loss and the gradient are bit for bit the default engine's, eager and captured
    (the generic kernels with all starts 0 run the plain kernels' arithmetic in the plain kernels' order)"""
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, V - 1, (B, T), generator=g)
    x[x == SEP] = V - 1
    y = torch.randint(0, V, (B, T), generator=g)
    for graph in (False, True):
        res = []
        for kw in ({}, {"doc_separator": SEP}):
            _, eng = _engine(dev, "fp32", graph, p=0.1, **kw)
            eng.set_batch(x.to(dev), y.to(dev))
            loss = eng.step().item()
            torch.cuda.synchronize()
            ev = eng.eval_loss(x.to(dev), y.to(dev)).item()
            res.append((loss, ev, _grads(eng)))
        assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
        _same_grads(res[0][2], res[1][2], exact_tok=False)


def test_evaluation_applies_the_mask(dev):
    """eval_loss and eval_losses of an engine with doc_separator: the module path's masked loss in eval() mode (1e-5, the bound of
    the two paths in tests/test_gpu_engine.py), not the default engine's"""
    corpus = _corpus()
    m, eng = _engine(dev, "fp32", True, doc_separator=SEP)
    _, plain = _engine(dev, "fp32", True)
    offs = torch.randint(0, 6000 - T - 1, (2, B), generator=torch.Generator().manual_seed(8))
    got = eng.eval_losses(corpus.to(dev), offs.to(dev)).cpu()
    m.eval().set_doc_separator(SEP)
    for i, r in enumerate(offs):
        x = torch.stack([corpus[o:o + T] for o in r.tolist()]).to(dev)
        y = torch.stack([corpus[o + 1:o + T + 1] for o in r.tolist()]).to(dev)
        want = m(x, y)[1].item()
        assert abs(got[i].item() - want) < 1e-5 and abs(eng.eval_loss(x, y).item() - want) < 1e-5
        assert abs(plain.eval_loss(x, y).item() - want) > 2e-5 * want
    # a batch of another size than the engine's own
    x1, y1 = x[:2].contiguous(), y[:2].contiguous()
    assert abs(eng.eval_loss(x1, y1).item() - m(x1, y1)[1].item()) < 1e-5


def test_state_dict_carries_the_option(dev):
    """meta.doc_separator is written only where set; a state without it loads into an engine with it and the reverse (the mask
    changes no state); two different separators are refused; a separator outside [0, V) is refused at construction"""
    from drakegpt_amd import checkpoint as CK
    _, A = _engine(dev, "fp32", False, doc_separator=SEP)
    _, Pn = _engine(dev, "fp32", False)
    x, y = _batch()
    A.set_batch(x.to(dev), y.to(dev))
    A.step()
    sd, plain = A.state_dict(), Pn.state_dict()
    assert sd["meta"]["doc_separator"] == SEP and "doc_separator" not in plain["meta"]
    _, B2 = _engine(dev, "fp32", False, doc_separator=SEP)
    B2.load_state_dict(sd)
    assert torch.equal(B2.flat, A.flat) and B2.state_dict()["meta"]["doc_separator"] == SEP
    Pn.load_state_dict(sd)                         # with -> without
    B2.load_state_dict(plain)                      # without -> with
    _, Cn = _engine(dev, "fp32", False, doc_separator=SEP + 1)
    before = Cn.flat.clone()
    with pytest.raises(ValueError, match=r"meta\.doc_separator differs.*saved 7.*8"):
        Cn.load_state_dict(sd)
    assert torch.equal(Cn.flat, before)
    for bad in (-1, V, True, 2.0):
        with pytest.raises(ValueError, match="doc_separator"):
            _engine(dev, "fp32", False, doc_separator=bad)
    assert CK is not None


def test_generate_does_not_apply_the_mask(dev):
    """with a separator set generate returns the tokens it returns without: host loop, cached loop and the graph-replayed device
    loop; the prompt holds the separator"""
    m = _model(dev, "fp32").eval()
    prompt = torch.tensor([[3, SEP, 5, 9, SEP, 2], [SEP, 4, 4, 6, 1, SEP]], device=dev)
    calls = [dict(use_cache=False), dict(use_cache=True), dict(use_cache=True, sampler="device", seed=5), dict(use_cache=False, sampler="device", seed=5)]
    want = []
    for kw in calls:
        gen = torch.Generator().manual_seed(0)
        want.append(m.generate(prompt.clone(), 12, generator=gen, **kw))
    m.set_doc_separator(SEP)
    for kw, w in zip(calls, want):
        gen = torch.Generator().manual_seed(0)
        assert torch.equal(m.generate(prompt.clone(), 12, generator=gen, **kw), w), kw
    assert m.doc_separator == SEP                                              # (generate put the option back)
    assert "stop_tokens=[sep]" in type(m).generate.__doc__ and "stop_tokens=[sep]" in type(m).__mro__[2].generate.__doc__


def test_train_harness_with_doc_separator(dev, tmp_path, capsys):
    """4 iterations on each training path with --doc-separator: the header names the separator, the evaluation lines are there and
    sane; a character is looked up in the tokenizer's table, and one that is not in the vocabulary is named in the error"""
    from drakegpt_amd import train
    from drakegpt_amd.config import DRAKE_VOCAB_SIZE
    flags = ["--doc-separator", "3", "--iters", "4", "--eval-interval", "2", "--eval-iters", "2", "--precision", "fp32", "--no-save",
             "--sample", "3"]
    for model in ("TransformerLM", "BlocksLM"):
        train.main(["--model", model] + flags)
        out = capsys.readouterr().out
        assert any("Document separator: token 3" in ln for ln in out.splitlines() if ln.startswith("Selected"))
        lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
        assert len(lines) == 2 and all(abs(ln["val_loss"] - math.log(DRAKE_VOCAB_SIZE)) < 0.5 for ln in lines), lines
    text = tmp_path / "songs.txt"
    text.write_text(("la la la di da\ndum di dum\n|" * 400))
    train.main(["--model", "BlocksLM", "--data", str(text), "--doc-separator", "|"] + flags[2:])
    out = capsys.readouterr().out
    vocab = sorted(set(text.read_text()))
    assert any(f"Document separator: token {vocab.index('|')}" in ln for ln in out.splitlines() if ln.startswith("Selected"))
    with pytest.raises(SystemExit, match=r"character '#' is not in the vocabulary"):
        train.main(["--model", "BlocksLM", "--data", str(text), "--doc-separator", "#"] + flags[2:])
    with pytest.raises(SystemExit, match=r"outside the vocabulary"):
        train.main(["--model", "BlocksLM", "--doc-separator", "100000"] + flags[2:])
    assert D is not None
