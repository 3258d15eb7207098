"""GPU: the exponential moving average of the weights inside the AdamW launch (dg_adamw_step_ema), dg_swap_f32, and
TrainEngine(ema_decay=) / optim.AdamW(ema_decay=) / train --ema-decay on top of them.

Kernel level: p, m, v, the bf16 shadow and the state words are compared bit for bit with dg_adamw_step_sched's, and the average bit
for bit with tests/ema_model.py (three separately rounded fp32 operations) applied to (old average, new p).  The sizes are those of
test_gpu_schedule.py: n = 2048 * 256 * 4 + 64 * 5 + 3 takes the grid-stride loop round a second time, has a scalar tail of 3 elements
and a partial last granule; n = 67 is one partial workgroup.

Engine level: the tiny fixture (C 32, T 8, 3 layers, fp32) for the recurrence -- which takes the OBSERVED weights as its input, so
the free order of the embedding atomics of that configuration does not matter -- and the widths of test_gpu_resume.py (V 80, C 384,
6 heads, T 256, B 8, 2 layers, bf16 / fp8), where the step has no atomics, for everything that compares two runs bit for bit."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_model as EM  # noqa: E402

pytestmark = pytest.mark.gpu
V = 80
BETAS = (0.9, 0.95)
N_BIG = 2048 * 256 * 4 + 64 * 5 + 3
SIZES = [N_BIG, 67]
HYPER = [1e-3, 0.9, 0.95, 1e-8, 0.1]


def _same(a, b):
    """bit equality of two tensors of the same dtype (NaN payloads and signed zeros included)"""
    it = {4: torch.int32, 2: torch.int16, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------ kernel
@pytest.fixture(scope="module")
def base(dev):
    """p, g, m, v and an old average of both sizes, made once and never written (every run works on clones)"""
    out = {}
    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        out[n] = tuple(t.to(dev) for t in (torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g),
                                            0.01 * torch.randn(n, generator=g), 1e-4 * torch.rand(n, generator=g),
                                            torch.randn(n, generator=g)))
    return out


def _combos(n, dev):
    """the eight clip / table / bitmap combinations"""
    from drakegpt_amd import ops
    table = torch.tensor([7e-4, 1e-3, 2.5e-4], dtype=torch.float32, device=dev)
    ng = (n + 63) // 64
    granules = torch.nonzero(torch.rand(ng, generator=torch.Generator().manual_seed(7)) < 0.5).flatten().tolist()
    bits = ops.new_no_decay_bits([(64 * G, min(64 * G + 64, n)) for G in granules], n, dev)
    return [(c, t, b) for c in (None, 0.37) for t in (None, table) for b in (None, bits)]


def _launch(base, n, dev, entry, *, step, clip=None, table=None, bits=None, advance=False, ema=None, hyper2=None, scale=0.5):
    """one launch on clones: entry "sched" is dg_adamw_step_sched, "ema" dg_adamw_step_ema with the same remaining arguments"""
    from drakegpt_amd import ops
    p, g, m, v = (t.clone() for t in base[n][:4])
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    state = ops.new_rng_state(123, dev, step)
    hy = torch.tensor(HYPER, dtype=torch.float32, device=dev)
    coef = None if clip is None else torch.tensor([clip], dtype=torch.float32, device=dev)
    head = (ops._p(p), ops._p(g), ops._p(m), ops._p(v), n, ops._p(hy), ops._p(state), scale, ops._p(coef), ops._p(table),
            0 if table is None else table.numel(), ops._p(bits), ops._p(shadow), int(advance))
    if entry == "sched":
        ops.check(ops.lib.dg_adamw_step_sched(*head, ops._stream()), "dg_adamw_step_sched")
    else:
        ops.check(ops.lib.dg_adamw_step_ema(*head, ops._p(ema), ops._p(hyper2), ops._stream()), "dg_adamw_step_ema")
    torch.cuda.synchronize()
    assert torch.equal(g, base[n][1])
    return {"p": p, "m": m, "v": v, "shadow": shadow, "state": state}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("s", [0, 1, 7])
def test_everything_but_the_average_is_the_sched_entry_and_the_average_is_the_model(dev, base, n, s):
    from drakegpt_amd import ops
    decay = 0.99
    hyper2 = ops.new_ema_hyper(decay, False, dev)
    old = base[n][4]
    old_np = old.cpu().numpy()
    for advance in (False, True):
        for clip, table, bits in _combos(n, dev):
            what = (s, advance, clip is not None, table is not None, bits is not None)
            ema = old.clone()
            got = _launch(base, n, dev, "ema", step=s, clip=clip, table=table, bits=bits, advance=advance, ema=ema, hyper2=hyper2)
            want = _launch(base, n, dev, "sched", step=s, clip=clip, table=table, bits=bits, advance=advance)
            for k in ("p", "m", "v", "shadow"):
                assert _same(got[k], want[k]), (what, k)
            assert got["state"].tolist() == want["state"].tolist() and got["state"].tolist()[2:] == [s + int(advance), 0], what
            assert not _same(got["p"], base[n][0])
            model = EM.step(old_np, got["p"].cpu().numpy(), decay, False, s)
            assert np.array_equal(_bits(ema), model.view(np.uint32)), what
            assert _same(hyper2, ops.new_ema_hyper(decay, False, dev))          # (read only)
    if s > 0:
        assert not _same(ema, got["p"]) and not _same(ema, old)


@pytest.mark.parametrize("n", SIZES)
def test_step_word_zero_does_not_read_the_buffer(dev, base, n):
    from drakegpt_amd import ops
    for warm in (False, True):
        ema = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
        got = _launch(base, n, dev, "ema", step=0, advance=True, ema=ema, hyper2=ops.new_ema_hyper(0.9, warm, dev))
        assert _same(ema, got["p"]) and bool(torch.isfinite(ema).all())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("s", [1, 5, 89])
def test_warmup_by_the_step_word(dev, base, n, s):
    """decay 0.9: d_1 = 2 / 11, d_5 = 0.4, d_89 = 0.9 (90 / 99 > 0.9: the decay itself)"""
    from drakegpt_amd import ops
    old = base[n][4]
    ema = old.clone()
    got = _launch(base, n, dev, "ema", step=s, ema=ema, hyper2=ops.new_ema_hyper(0.9, True, dev))
    p = got["p"].cpu().numpy()
    assert np.array_equal(_bits(ema), EM.step(old.cpu().numpy(), p, 0.9, True, s).view(np.uint32))
    plain = EM.step(old.cpu().numpy(), p, 0.9, False, s)
    assert np.array_equal(_bits(ema), plain.view(np.uint32)) == (s == 89)          # (the warm-up did change the result before step 81)
    assert EM.decay_at(0.9, True, s) == {1: np.float32(2) / np.float32(11), 5: np.float32(0.4), 89: np.float32(0.9)}[s]


@pytest.mark.parametrize("n", SIZES)
def test_three_chained_launches_and_a_new_decay_under_a_captured_graph(dev, base, n):
    from drakegpt_amd import ops
    p, g, m, v = (t.clone() for t in base[n][:4])
    ema = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    state = ops.new_rng_state(5, dev, 0)
    hy = torch.tensor(HYPER, dtype=torch.float32, device=dev)
    hyper2 = ops.new_ema_hyper(0.9, True, dev)
    model, seen = None, []
    for s in range(3):                                   # through the wrapper, the step word moved on by the launch itself
        ops.adamw_step(p, g, m, v, hy, state, 0.5, n=n, advance=True, ema=ema, ema_hyper=hyper2)
        seen.append(p.cpu().numpy())
        model = EM.step(model, seen[-1], 0.9, True, s)
    assert state.tolist()[2:] == [3, 0] and np.array_equal(_bits(ema), model.view(np.uint32))
    assert not np.array_equal(seen[0], seen[2])
    # one captured launch, replayed: the decay is read from device memory at every replay
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        ops.adamw_step(p, g, m, v, hy, state, 0.5, n=n, advance=True, ema=ema, ema_hyper=hyper2)
    for s, (decay, warm) in zip((3, 4, 5), ((0.9, True), (0.5, True), (0.25, False))):
        hyper2.copy_(ops.new_ema_hyper(decay, warm, dev))
        graph.replay()
        torch.cuda.synchronize()
        model = EM.step(model, p.cpu().numpy(), decay, warm, s)
        assert np.array_equal(_bits(ema), model.view(np.uint32)), (s, decay, warm)
    assert state.tolist()[2:] == [6, 0]


@pytest.mark.parametrize("n", SIZES)
def test_swap(dev, base, n):
    from drakegpt_amd import ops
    a0, b0 = base[n][0], base[n][4]
    a, b = a0.clone(), b0.clone()
    a[0], b[n - 1] = float("nan"), -0.0
    a0, b0 = a.clone(), b.clone()
    ops.swap_(a, b)
    assert _same(a, b0) and _same(b, a0) and not _same(a, a0)
    ops.swap_(a, b)
    assert _same(a, a0) and _same(b, b0)
    ops.swap_(a, b, n=n - 3 if n > 67 else 5)            # a prefix only
    k = n - 3 if n > 67 else 5
    assert _same(a[:k], b0[:k]) and _same(a[k:], a0[k:]) and _same(b[:k], a0[:k]) and _same(b[k:], b0[k:])
    err_arg = ops.lib.dg_swap_f32(None, ops._p(b), n, ops._stream())
    assert err_arg != 0 and ops.lib.dg_swap_f32(ops._p(a), None, n, ops._stream()) == err_arg
    assert ops.lib.dg_swap_f32(ops._p(a), ops._p(b), 0, ops._stream()) == err_arg
    err_align = ops.lib.dg_adamw_step(a.data_ptr() + 4, ops._p(a), ops._p(a), ops._p(a), 8, ops._p(a), ops._p(a), 1.0, None, 0, ops._stream())
    assert err_align not in (0, err_arg)
    assert ops.lib.dg_swap_f32(a.data_ptr() + 4, ops._p(b), 8, ops._stream()) == err_align
    assert ops.lib.dg_swap_f32(ops._p(a), b.data_ptr() + 8, 8, ops._stream()) == err_align
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="overlap"):
        ops.swap_(a, a)
    with pytest.raises(ValueError, match="does not fit"):
        ops.swap_(a, b, n=n + 1)
    with pytest.raises(TypeError, match="must be"):
        ops.swap_(a, b.double())


def test_argument_checks(dev, base):
    from drakegpt_amd import ops
    n = 67
    p, g, m, v, ema = (t.clone() for t in base[n])
    hy = torch.tensor(HYPER, device=dev)
    state = ops.new_rng_state(1, dev, 0)
    table = torch.tensor([1e-3, 2e-3], device=dev)
    h2 = ops.new_ema_hyper(0.9, False, dev)

    def call(pp=ops._p(p), tab=None, length=0, e=ops._p(ema), hh=ops._p(h2), nn=n):
        return ops.lib.dg_adamw_step_ema(pp, ops._p(g), ops._p(m), ops._p(v), nn, ops._p(hy), ops._p(state), 1.0, None, tab, length,
                                         None, None, 0, e, hh, ops._stream())
    err_arg = ops.lib.dg_adamw_step(None, ops._p(g), ops._p(m), ops._p(v), n, ops._p(hy), ops._p(state), 1.0, None, 0, ops._stream())
    err_align = ops.lib.dg_adamw_step(p.data_ptr() + 4, ops._p(g), ops._p(m), ops._p(v), 8, ops._p(hy), ops._p(state), 1.0, None, 0, ops._stream())
    assert err_arg != 0 and err_align not in (0, err_arg)
    # what dg_adamw_step_sched refuses ...
    assert call(pp=None) == err_arg and call(nn=0) == err_arg
    assert call(tab=None, length=2) == err_arg and call(tab=ops._p(table), length=0) == err_arg and call(tab=ops._p(table), length=-1) == err_arg
    assert call(pp=p.data_ptr() + 4, nn=8) == err_align
    # ... a NULL average, NULL options, a misaligned average
    assert call(e=None) == err_arg and call(hh=None) == err_arg
    assert call(e=ema.data_ptr() + 4, nn=8) == err_align
    torch.cuda.synchronize()
    assert _same(p, base[n][0]) and _same(ema, base[n][4])          # nothing was launched
    assert call() == 0 and call(tab=ops._p(table), length=2) == 0
    torch.cuda.synchronize()
    # the wrapper checks what the kernel would index
    with pytest.raises(ValueError, match="ema needs ema_hyper"):
        ops.adamw_step(p, g, m, v, hy, state, ema=ema)
    with pytest.raises(ValueError, match="ema_hyper goes with ema"):
        ops.adamw_step(p, g, m, v, hy, state, ema_hyper=h2)
    with pytest.raises(ValueError, match="does not fit"):
        ops.adamw_step(p, g, m, v, hy, state, ema=ema[:64], ema_hyper=h2)
    with pytest.raises(ValueError, match="2 floats"):
        ops.adamw_step(p, g, m, v, hy, state, ema=ema, ema_hyper=h2[:1])
    with pytest.raises(TypeError, match="ema"):
        ops.adamw_step(p, g, m, v, hy, state, ema=ema.double(), ema_hyper=h2)
    with pytest.raises(ValueError, match="no_decay_bits needs"):
        ops.adamw_step(*base[N_BIG][:4], hy, state, n=64 * 33, no_decay_bits=ops.new_no_decay_bits([], n, dev), ema=base[N_BIG][4], ema_hyper=h2)


# ------------------------------------------------------------------------------------------------ engine, tiny fixture
@pytest.fixture(scope="module")
def fix(golden_dir):
    return torch.load(os.path.join(golden_dir, "traj5_TransformerLM.pt"), weights_only=True)


def _tiny(dev, fix, B, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    m.load_state_dict(fix["init"])
    m = m.to(dev).train()
    kw.setdefault("lr", 1e-3)
    return m, TrainEngine(m, B, 8, betas=BETAS, **kw)


def _one_sequence_batch(i, B, dev):
    row = torch.randperm(V, generator=torch.Generator().manual_seed(100 + i))[:9]
    return row[:8].repeat(B, 1).to(dev), row[1:9].repeat(B, 1).to(dev)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("accum", [1, 2])
def test_engine_average_follows_the_optimizer_steps(dev, fix, graph, accum):
    """five optimizer steps: `ema` is the model run over the flat images read back after each step, bit for bit; under accum_steps
    = 2 it does not move on a non-final micro-step; ema_state_dict() is what an AveragedModel fed the same weights holds, within
    2 k 2^-24 max|p| (tests/test_ema_host.py), under the reference's parameter names -- q / k / v rows included"""
    import drakegpt_amd as D
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    decay, steps, B = 0.9, 5, 32 // accum
    m, eng = _tiny(dev, fix, B, use_graph=graph, accum_steps=accum, ema_decay=decay)
    assert eng.ema.shape == (eng.n_active,) and _same(eng.ema, eng.flat[:eng.n_active]) and eng.ema_hyper.tolist() == [np.float32(decay), 0.0]
    assert eng.ema.data_ptr() != eng.flat.data_ptr()
    plain = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    plain.load_state_dict(fix["init"])
    avg = AveragedModel(plain, multi_avg_fn=get_ema_multi_avg_fn(decay))
    model, top = None, 0.0
    for s in range(steps):
        for j in range(accum):
            before = eng.ema.clone()
            x, y = _one_sequence_batch(s * accum + j, B, dev)
            eng.set_batch(x, y)
            eng.micro_step() if accum > 1 else eng.step()
            torch.cuda.synchronize()
            if j < accum - 1:
                assert _same(eng.ema, before), (s, j)
        flat = eng.flat[:eng.n_active].cpu().numpy()
        model = EM.step(model, flat, decay, False, s)
        assert np.array_equal(_bits(eng.ema), model.view(np.uint32)), s
        top = max(top, float(np.abs(flat).max()))
        plain.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
        avg.update_parameters(plain)
    assert eng.step_count() == steps and eng.micro_step_count() == steps * accum
    assert not _same(eng.ema, eng.flat[:eng.n_active])
    bound = 2 * steps * 2.0 ** -24 * top
    got, want = eng.ema_state_dict(), avg.module.state_dict()
    names = [k for k, _ in plain.named_parameters()]
    assert set(names) <= set(got) and set(got) == set(m.state_dict())
    worst = 0.0
    for k in names:
        assert got[k].device.type == "cpu" and got[k].shape == want[k].shape, k
        worst = max(worst, float((got[k].double() - want[k].double()).abs().max()))
    print(f"graph {graph} accum {accum}: ema_state_dict vs AveragedModel {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    # a wrong row mapping would miss by the distance between two heads' weights
    q0, k0 = got["blocks.0.sa_head.heads.0.query.weight"], got["blocks.0.sa_head.heads.0.key.weight"]
    assert float((q0 - k0).abs().max()) > 1000 * bound
    assert _same(eng.ema_view("1.w1"), eng.ema[eng._region("1.w1")[0]:][:eng.param_view("1.w1").numel()].view(eng.param_view("1.w1").shape))
    fresh = D.TransformerLM(V, 32, 8, 4, 3, 0.0)
    fresh.load_state_dict(got)                           # loads into a plain model


def test_default_engine_never_calls_the_new_entry(dev, fix, monkeypatch):
    """(g) the monkeypatch of test_gpu_schedule.py::test_default_engine_makes_the_adamw_call_it_always_made: a default engine passes no
    new keyword and never reaches dg_adamw_step_ema; an engine with ema_decay does"""
    from drakegpt_amd import ops
    real, real_entry, calls = ops.adamw_step, ops.lib.dg_adamw_step_ema, []

    def entry(*a):
        calls.append(len(a))
        return real_entry(*a)
    monkeypatch.setattr(ops.lib, "dg_adamw_step_ema", entry)

    def earlier(p, g, m, v, hyper, rng_state, grad_scale=1.0, shadow_bf16=None, n=None, advance=False, *, clip=None):
        return real(p, g, m, v, hyper, rng_state, grad_scale, shadow_bf16, n, advance, clip=clip)
    monkeypatch.setattr(ops, "adamw_step", earlier)
    for kw in ({}, {"max_grad_norm": 1.0}, {"accum_steps": 2}):
        _, eng = _tiny(dev, fix, 16, use_graph=False, **kw)
        assert eng.ema is None and eng.ema_hyper is None and eng._ema_kw == {}
        x, y = _one_sequence_batch(0, 16, dev)
        for _ in range(eng.accum):
            eng.set_batch(x, y)
            eng.micro_step() if eng.accum > 1 else eng.step()
        assert eng.step_count() == 1
    assert calls == []
    monkeypatch.setattr(ops, "adamw_step", real)
    for i, kw in enumerate(({}, {"max_grad_norm": 1.0}, {"accum_steps": 2})):
        _, eng = _tiny(dev, fix, 16, use_graph=False, ema_decay=0.9, **kw)
        x, y = _one_sequence_batch(0, 16, dev)
        for _ in range(eng.accum):
            eng.set_batch(x, y)
            eng.micro_step() if eng.accum > 1 else eng.step()
        assert eng.step_count() == 1 and calls == [17] * (i + 1)


def test_constructor_and_setter(dev, fix):
    for kw in (dict(ema_decay=1.0), dict(ema_decay=0.0), dict(ema_decay=True), dict(ema_decay=float("nan")), dict(ema_warmup=True)):
        with pytest.raises(ValueError, match="ema_"):
            _tiny(dev, fix, 32, **kw)
    _, eng = _tiny(dev, fix, 32, ema_decay=0.9, ema_warmup=True, use_graph=True)
    assert eng.ema_hyper.tolist() == [np.float32(0.9), 1.0]
    x, y = _one_sequence_batch(0, 32, dev)
    eng.set_batch(x, y)
    eng.step()
    graphs, ptr = eng._graphs, eng.ema_hyper.data_ptr()
    eng.set_ema_decay(0.5)
    assert eng.ema_decay == 0.5 and eng.ema_hyper.tolist() == [0.5, 1.0] and eng.ema_hyper.data_ptr() == ptr and eng._graphs is graphs
    old = eng.ema.cpu().numpy()
    eng.step()
    torch.cuda.synchronize()
    assert eng._graphs is graphs
    want = EM.step(old, eng.flat[:eng.n_active].cpu().numpy(), 0.5, True, 1)          # d_1 = min(0.5, 2 / 11)
    assert np.array_equal(_bits(eng.ema), want.view(np.uint32))
    for bad in (1.0, None, True):
        with pytest.raises(ValueError, match="ema_decay|decay must be"):
            eng.set_ema_decay(bad)
    _, plain = _tiny(dev, fix, 32)
    for call in (lambda: plain.set_ema_decay(0.9), lambda: plain.ema_view("lm.w"), plain.ema_state_dict):
        with pytest.raises(RuntimeError, match="without a moving average"):
            call()


# ------------------------------------------------------------------------------------------------ no atomics: bit for bit
RV, RC, RNH, RT, RB, RP, RL = 80, 384, 6, 256, 8, 0.2, 2
N_CORPUS = 20_000


def _corpus():
    return torch.randint(0, RV, (N_CORPUS,), generator=torch.Generator().manual_seed(1))


def _rows(n, seed=2):
    return torch.randint(0, N_CORPUS - RT - 1, (n, RB), generator=torch.Generator().manual_seed(seed))


def _scaled(dev, precision="bf16", model_seed=42, seed=20240607, weights=None, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    torch.manual_seed(model_seed)
    m = D.TransformerLM(RV, RC, RT, RNH, RL, RP, precision=precision)
    if weights is not None:
        m.load_state_dict(weights)
    m = m.to(dev).train()
    eng = TrainEngine(m, RB, RT, lr=3e-4, betas=BETAS, seed=seed, use_graph=True, **kw)
    assert eng.onehot is not None and eng.grouped_dw            # no atomics in the step: bit-reproducible across engines
    eng.set_corpus(_corpus().to(dev))
    return m, eng


def test_training_is_unchanged_by_the_average(dev):
    """(a)"""
    _, A = _scaled(dev, ema_decay=0.99)
    _, Bn = _scaled(dev)
    losses = []
    for e in (A, Bn):
        e.stage_offsets(_rows(4))
        losses.append([e.step().item() for _ in range(4)])
    torch.cuda.synchronize()
    assert losses[0] == losses[1] and len(set(losses[0])) == 4
    for k in ("flat", "m_", "v_", "shadow"):
        assert _same(getattr(A, k), getattr(Bn, k)), k


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_evaluation_inside_the_context_sees_the_average(dev, precision):
    """(b)"""
    from drakegpt_amd import ops
    m, A = _scaled(dev, precision, ema_decay=0.9)
    A.stage_offsets(_rows(3))
    for _ in range(3):
        A.step()
    data, offs = _corpus().to(dev), _rows(2, seed=11).to(dev)
    raw = A.eval_losses(data, offs).clone()
    sd = A.ema_state_dict()
    flat, ema = A.flat.clone(), A.ema.clone()
    with A.ema_weights() as inside:
        assert inside is A and _same(A.flat[:A.n_active], ema) and _same(A.ema, flat[:A.n_active]) and _same(A.flat[A.n_active:], flat[A.n_active:])
        avg = A.eval_losses(data, offs).clone()
        seen = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        x, y = ops.batch_gather(data, offs[0], RT)
        one = A.eval_loss(x, y).clone()
    torch.cuda.synchronize()
    assert _same(A.flat, flat) and _same(A.ema, ema)
    assert seen.keys() == sd.keys() and all(_same(seen[k], sd[k]) for k in sd)          # model.state_dict() inside == ema_state_dict()
    _, Bn = _scaled(dev, precision, model_seed=3, seed=9, weights=sd)
    assert _same(Bn.flat[:Bn.n_active], ema)
    ref = Bn.eval_losses(data, offs)
    torch.cuda.synchronize()
    print(f"{precision}: raw {raw.tolist()} averaged {avg.tolist()}")
    assert _same(avg, ref), (avg.tolist(), ref.tolist())
    assert one.item() == avg[0].item()
    assert all(a != r for a, r in zip(avg.tolist(), raw.tolist()))
    assert _same(A.eval_losses(data, offs), raw)                                          # and the raw weights' loss is back


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_the_swap_restores_the_run(dev, precision):
    """(c)"""
    data, offs = _corpus().to(dev), _rows(2, seed=11).to(dev)
    out = []
    for use_context in (True, False):
        _, E = _scaled(dev, precision, ema_decay=0.99)
        E.stage_offsets(_rows(4))
        losses = [E.step().item() for _ in range(2)]
        if use_context:
            with E.ema_weights():
                E.eval_losses(data, offs)
        else:
            E.eval_losses(data, offs)
        losses += [E.step().item() for _ in range(2)]
        torch.cuda.synchronize()
        E.check_status()
        out.append((E, losses))
    (A, la), (Bn, lb) = out
    assert la == lb and len(set(la)) == 4, (la, lb)
    for k in ("flat", "m_", "v_", "ema", "shadow"):
        assert _same(getattr(A, k), getattr(Bn, k)), k


def test_refused_calls_inside_the_context(dev):
    """(d)"""
    _, A = _scaled(dev, ema_decay=0.99)
    A.stage_offsets(_rows(2))
    A.step()
    sd = A.state_dict()
    flat = A.flat.clone()
    with A.ema_weights():
        for what, call in (("step", A.step), ("micro_step", A.micro_step), ("state_dict", A.state_dict),
                           ("load_state_dict", lambda: A.load_state_dict(sd)),
                           ("load_optimizer_state_dict", lambda: A.load_optimizer_state_dict(sd["optimizer"])),
                           ("ema_weights", lambda: A.ema_weights().__enter__())):
            with pytest.raises(RuntimeError, match=what + r"\(\) inside"):
                call()
    assert not A._in_ema and _same(A.flat, flat)
    with pytest.raises(KeyError):                        # an exception inside still swaps back
        with A.ema_weights():
            raise KeyError("x")
    assert not A._in_ema and _same(A.flat, flat)
    A.step()
    _, plain = _scaled(dev)
    with pytest.raises(RuntimeError, match="without a moving average"):
        with plain.ema_weights():
            pass


PARENT_ENGINE_KEYS = {"seed", "step_word", "opt_step", "acc_ctl", "max_grad_norm", "offsets", "offsets_rows", "offsets_left", "fp8_seeded",
                      "fp8_sites", "lr_table", "no_decay"}
PARENT_META_KEYS = {"precision", "vocab_size", "embedding_dim", "num_layers", "num_heads", "model_context_length", "batch_size",
                    "context_length", "accum_steps", "world_size", "dropout"}


@pytest.mark.parametrize("accum", [1, 2])
def test_resume_into_a_fresh_engine(dev, tmp_path, accum):
    """(e) the path of train --resume: construct, load, then step.  The first step after the load captures at step word 2, so the
    capture's warm-up launch moves the average (s > 0: it is read and averaged, not overwritten as at step word 0) and only the
    snapshot the capture takes of `ema` puts it back.  Checked twice: the first step after the load against the recurrence on
    the file's average (a lost restore would have averaged the warm-up's weights in as well), and three steps against the
    uninterrupted run, bit for bit."""
    from drakegpt_amd import checkpoint as CK
    kw = dict(accum_steps=accum)
    _, A = _scaled(dev, ema_decay=0.9, ema_warmup=True, **kw)
    A.stage_offsets(_rows(5 * accum))
    for _ in range(2):
        A.step()
    path = str(tmp_path / "ema.state.pt")
    CK.save_train_state(path, A.state_dict())
    sd = CK.load_train_state(path)
    saved = sd["engine"]["ema"]["values"].numpy().copy()
    la = [A.step().item() for _ in range(3)]
    # other initial weights, dropout seed, decay and no warm-up: the file's replace them; no step and no capture before the load
    _, Bn = _scaled(dev, model_seed=7, seed=99, ema_decay=0.5, **kw)
    assert Bn._graphs is None
    Bn.load_state_dict(sd)
    assert Bn._graphs is None and Bn.step_count() == 2 and (Bn.ema_decay, Bn.ema_warmup) == (0.9, True)
    assert np.array_equal(_bits(Bn.ema), saved.view(np.uint32)) and not _same(Bn.ema, Bn.flat[:Bn.n_active])
    lb = [Bn.step().item()]
    torch.cuda.synchronize()
    assert Bn._graphs is not None and Bn.step_count() == 3
    want = EM.step(saved, Bn.flat[:Bn.n_active].cpu().numpy(), 0.9, True, 2)
    assert np.array_equal(_bits(Bn.ema), want.view(np.uint32))
    lb += [Bn.step().item() for _ in range(2)]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for k in ("flat", "m_", "v_", "ema", "shadow"):
        assert _same(getattr(A, k), getattr(Bn, k)), k
    assert A.step_count() == Bn.step_count() == 5 and A.micro_step_count() == Bn.micro_step_count() == 5 * accum


def test_resume_and_the_state_of_a_default_engine(dev, tmp_path):
    """(e) into a running engine, (f)"""
    from drakegpt_amd import checkpoint as CK
    _, A = _scaled(dev, ema_decay=0.9, ema_warmup=True)
    A.stage_offsets(_rows(5))
    for _ in range(2):
        A.step()
    path = str(tmp_path / "ema.state.pt")
    CK.save_train_state(path, A.state_dict())
    sd = CK.load_train_state(path)                                 # torch.load(..., weights_only=True)
    assert sd["meta"]["ema"] is True and set(sd["meta"]) == PARENT_META_KEYS | {"ema"} and set(sd["engine"]) == PARENT_ENGINE_KEYS | {"ema"}
    assert sd["engine"]["ema"]["decay"] == 0.9 and sd["engine"]["ema"]["warmup"] is True and _same(sd["engine"]["ema"]["values"], A.ema.cpu())
    la = [A.step().item() for _ in range(3)]
    # a running engine with other weights, another decay and no warm-up: the file's replace them, in place
    _, Bn = _scaled(dev, model_seed=7, seed=99, ema_decay=0.5)
    Bn.stage_offsets(_rows(1, seed=9))
    Bn.step()
    graphs, ptrs = Bn._graphs, (Bn.ema.data_ptr(), Bn.ema_hyper.data_ptr())
    assert graphs is not None
    Bn.load_state_dict(sd)
    assert Bn._graphs is graphs and (Bn.ema.data_ptr(), Bn.ema_hyper.data_ptr()) == ptrs
    assert (Bn.ema_decay, Bn.ema_warmup) == (0.9, True) and Bn.ema_hyper.tolist() == [np.float32(0.9), 1.0] and Bn.step_count() == 2
    lb = [Bn.step().item() for _ in range(3)]
    torch.cuda.synchronize()
    assert la == lb, (la, lb)
    for k in ("flat", "m_", "v_", "ema", "shadow"):
        assert _same(getattr(A, k), getattr(Bn, k)), k
    # (f) a default engine writes exactly the parent's keys; the presence of the average must agree in both directions
    _, Dn = _scaled(dev, model_seed=9, seed=6)
    plain = Dn.state_dict()
    assert set(plain["engine"]) == PARENT_ENGINE_KEYS and set(plain["meta"]) == PARENT_META_KEYS
    Dn.load_state_dict(plain)
    before = {k: getattr(Dn, k).clone() for k in ("flat", "m_", "v_", "state")}
    with pytest.raises(ValueError, match=r"meta\.ema differs.*True.*False"):
        Dn.load_state_dict(sd)
    assert all(_same(getattr(Dn, k), t) for k, t in before.items())
    before = {k: getattr(Bn, k).clone() for k in ("flat", "m_", "v_", "state", "ema", "ema_hyper")}
    with pytest.raises(ValueError, match=r"meta\.ema differs.*False.*True"):
        Bn.load_state_dict(plain)
    for bad, what in ((dict(sd, engine={k: v for k, v in sd["engine"].items() if k != "ema"}), r"engine\.ema differs"),
                      (dict(sd, engine=dict(sd["engine"], ema=dict(sd["engine"]["ema"], values=sd["engine"]["ema"]["values"][:-1]))),
                       r"engine\.ema\.values"),
                      (dict(sd, engine=dict(sd["engine"], ema=dict(sd["engine"]["ema"], decay=1.5))), r"engine\.ema\.decay")):
        with pytest.raises(ValueError, match=what):
            Bn.load_state_dict(bad)
    assert all(_same(getattr(Bn, k), t) for k, t in before.items())


# ------------------------------------------------------------------------------------------------ autograd path
def test_autograd_path(dev, fix, tmp_path):
    import drakegpt_amd as D
    from drakegpt_amd.optim import AdamW
    torch.manual_seed(5)
    mod = D.BlocksLM(V, 32, 8, 4, 3).to(dev).train()
    opt = AdamW(mod.parameters(), lr=1e-3, betas=BETAS, ema_decay=0.9)
    model = None
    for s in range(3):
        _, loss = mod(fix["x"][s].to(dev), fix["y"][s].to(dev))
        opt.zero_grad()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        fl = opt._flat[0]
        model = EM.step(model, fl.flat.cpu().numpy(), 0.9, False, s)
        assert np.array_equal(_bits(fl.ema), model.view(np.uint32)), s
    assert len(opt._flat) == 1 and not _same(fl.ema, fl.flat)
    flat, ema = fl.flat.clone(), fl.ema.clone()
    raw = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    with opt.ema_weights():
        assert _same(fl.flat, ema) and _same(fl.ema, flat)
        inside = {k: v.detach().clone() for k, v in mod.state_dict().items()}
        for what, call in (("step", opt.step), ("state_dict", opt.state_dict), ("ema_weights", lambda: opt.ema_weights().__enter__())):
            with pytest.raises(RuntimeError, match=what + r"\(\) inside"):
                call()
    assert _same(fl.flat, flat) and _same(fl.ema, ema)
    assert all(_same(v, raw[k]) for k, v in mod.state_dict().items()) and any(not _same(inside[k], raw[k]) for k in raw)
    i = [id(p) for p in mod.parameters()].index(id(mod.lm_head.weight))
    assert _same(inside["lm_head.weight"], fl.view(ema, fl.key.index(id(mod.lm_head.weight)), mod.lm_head.weight))
    # the state round-trips through a file, in torch.optim.AdamW's format plus one top-level key
    from drakegpt_amd.train import _to_cpu
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups", "ema"} and set(sd["ema"]["values"]) == set(sd["state"]) and i in sd["state"]
    path = str(tmp_path / "opt.pt")
    torch.save(_to_cpu(sd), path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    mod2 = D.BlocksLM(V, 32, 8, 4, 3).to(dev).train()
    mod2.load_state_dict(mod.state_dict())
    opt2 = AdamW(mod2.parameters(), lr=5e-3, ema_decay=0.5, ema_warmup=True)
    # a refused load leaves the options as they were
    bad = dict(sd, state={k: (dict(v, step=torch.tensor(9.0)) if k == i else v) for k, v in sd["state"].items()})
    with pytest.raises(ValueError, match="ONE step count"):
        opt2.load_state_dict(bad)
    assert (opt2.ema_decay, opt2.ema_warmup) == (0.5, True) and not opt2._flat
    opt2.load_state_dict(sd)
    f2 = opt2._flat[0]
    assert (opt2.ema_decay, opt2.ema_warmup) == (0.9, False) and f2.ema_hyper.tolist() == [np.float32(0.9), 0.0]
    assert int(f2.t[2]) == 3
    for k in ("flat", "m", "v", "ema"):
        assert _same(getattr(f2, k), getattr(fl, k)), k
    plain = AdamW(mod2.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="ema differs"):
        plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="ema differs"):
        opt2.load_state_dict({k: v for k, v in sd.items() if k != "ema"})


# ------------------------------------------------------------------------------------------------ harness
def _harness(capsys, argv):
    from drakegpt_amd import train
    train.main(argv)
    out = capsys.readouterr().out.splitlines()
    return [json.loads(s) for s in out if s.startswith("{") and '"val_loss"' in s], [s[len("saved "):] for s in out if s.startswith("saved ")]


def _harness_base(monkeypatch, model):
    """two runs are compared for equality, so both must be reproducible to the last bit.  TransformerLM: the no-atomics widths.
    BlocksLM (autograd path): its one order-dependent sum is the fp32 atomicAdd of the token-table gradient (dg_embed_bwd); the tiny
    preset at batch_size 2 puts 16 tokens into a training batch, and a table row that receives at most two contributions is
    0 + a + b in either order -- test_train_harness checks that on the batches the run really drew."""
    from drakegpt_amd import train
    from drakegpt_amd.config import PARAMS
    monkeypatch.setitem(train.PRESETS, "ema_test", {
        "context_length": RT, "batch_size": RB, "base_lr": 3e-4, "max_lr": 6e-4, "betas": BETAS, "embedding_dim": RC, "head_size": 64,
        "num_heads": RNH, "num_layers": RL, "dropout": RP})
    monkeypatch.setitem(train.PRESETS, "ema_tiny", dict(PARAMS, batch_size=2))
    if model == "TransformerLM":
        return ["--model", model, "--preset", "ema_test", "--precision", "bf16"]
    return ["--model", model, "--preset", "ema_tiny", "--precision", "fp32"]


@pytest.mark.parametrize("model", ["TransformerLM", "BlocksLM"])
def test_train_harness(dev, capsys, monkeypatch, tmp_path, model):
    """6 iterations, an evaluation every 2: the run with --ema-decay reports the train_loss / val_loss / lr of the run without it
    (nothing more is drawn from the host generator; the swap restores the weights)."""
    import drakegpt_amd as D
    from drakegpt_amd import train
    from drakegpt_amd.preprocessing import split_train_val
    base = _harness_base(monkeypatch, model)
    base += ["--iters", "6", "--eval-interval", "2", "--eval-iters", "2", "--sample", "3", "--model-dir", str(tmp_path)]
    real, draws = train.draw_offsets, []

    def recording(n, T, B, generator=None):
        draws.append(real(n, T, B, generator))
        return draws[-1]
    monkeypatch.setattr(train, "draw_offsets", recording)
    plain, _ = _harness(capsys, base + ["--no-save"])
    first = [d.clone() for d in draws]
    if model == "BlocksLM":
        # per interval of 2 iterations: 2 training draws, then 2 + 2 evaluation draws; every training batch of the synthetic corpus
        # holds each token at most twice (see _harness_base)
        corpus, _ = split_train_val(torch.randint(0, V, (1_000_000,), generator=torch.Generator().manual_seed(42)))
        assert len(first) == 18 and all(d.shape == (2,) for d in first)
        for k in (0, 1, 6, 7, 12, 13):
            toks = torch.cat([corpus[i:i + 8] for i in first[k].tolist()])
            assert int(torch.bincount(toks, minlength=V).max()) <= 2, k
    del draws[:]
    lines, saved = _harness(capsys, base + ["--ema-decay", "0.9", "--save-every", "6"])
    assert [ln["step"] for ln in lines] == [2, 4, 6] == [ln["step"] for ln in plain]
    assert len(draws) == len(first) and all(torch.equal(a, b) for a, b in zip(draws, first))          # the same draws, no extra one
    assert all(np.isfinite(ln["val_loss_ema"]) for ln in lines) and not any("val_loss_ema" in ln for ln in plain)
    for a, b in zip(lines, plain):
        print(model, a, b)
        for k in ("train_loss", "val_loss", "lr"):
            assert a[k] == b[k], (k, a, b)
    assert any(ln["val_loss_ema"] != ln["val_loss"] for ln in lines)
    name = os.path.join(str(tmp_path), model)
    assert saved == [name + ".ema.pt", name + ".pt"]
    raw, ema = (torch.load(name + ext, weights_only=True) for ext in (".pt", ".ema.pt"))
    assert raw.keys() == ema.keys() and any(not torch.equal(raw[k], ema[k]) for k in raw)
    cfg = dict(vocab_size=V, embedding_dim=RC, context_length=RT, num_heads=RNH, num_layers=RL, dropout=RP) if model == "TransformerLM" \
        else dict(vocab_size=V, embedding_dim=32, context_length=8, num_heads=4, num_layers=3)
    D.MODEL_CLASSES[model](**cfg).load_state_dict(ema)
    state = name + ".state.pt"
    assert os.path.isfile(state)
    monkeypatch.setattr(train, "draw_offsets", real)
    for other in (["--ema-decay", "0.5"], []):
        with pytest.raises(SystemExit, match="ema_decay differs"):
            train.main(base + other + ["--resume", state])


@pytest.mark.parametrize("model", ["TransformerLM", "BlocksLM"])
def test_train_harness_resume_continues_the_average(dev, capsys, monkeypatch, tmp_path, model):
    """--iters 6 against --iters 4 --save-every 4 followed by --resume --iters 6, all with --ema-decay: the resumed run's evaluation
    line, val_loss_ema included, and its <name>.ema.pt are the uninterrupted run's, bit for bit (both models run where a run is
    reproducible to the last bit: _harness_base; the draws are those test_train_harness checks)."""
    base = _harness_base(monkeypatch, model)
    base += ["--eval-interval", "2", "--eval-iters", "2", "--sample", "3", "--ema-decay", "0.9", "--ema-warmup"]
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    whole, _ = _harness(capsys, base + ["--iters", "6", "--model-dir", a])
    first, _ = _harness(capsys, base + ["--iters", "4", "--save-every", "4", "--model-dir", b])
    rest, _ = _harness(capsys, base + ["--iters", "6", "--resume", os.path.join(b, model + ".state.pt"), "--model-dir", b])
    assert [ln["step"] for ln in whole] == [2, 4, 6] and [ln["step"] for ln in first] == [2, 4] and [ln["step"] for ln in rest] == [6]
    ea, eb = (torch.load(os.path.join(d, model + ".ema.pt"), weights_only=True) for d in (a, b))
    assert ea.keys() == eb.keys()
    for x, y in zip(whole, first + rest):
        print(model, x, y)
        assert x["lr"] == y["lr"]
        for k in ("train_loss", "val_loss", "val_loss_ema"):
            assert x[k] == y[k], (k, x, y)
    assert all(torch.equal(ea[k], eb[k]) for k in ea)
    assert whole[-1]["val_loss_ema"] != whole[-1]["val_loss"]
