"""The update guard on the GPU: dg_grad_norm_finalize_guard and dg_adamw_step_guard against the unguarded entries and the numpy
model (tests/guard_model.py), then TrainEngine, optim.AdamW and the harness with the guard on.  Every comparison is between two runs
of this library on the same device and is exact: bits, no tolerance."""
import contextlib
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_model as GM  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
V = 80
BAND = 64
NAN, INF = float("nan"), float("inf")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ================================================================================================ finalize
NORM_SIZES = (1, 4099, 2048 * 4096 + 4096 + 3)          # one element; a tail; a second grid-stride trip, the cap on partials and the tail
CONTENTS = ("finite", "nan_first", "nan_middle", "nan_last", "pos_inf", "neg_inf", "big_3e19")


@pytest.fixture(scope="module")
def norm_buffers(dev):
    """one finite buffer per size, made once; a case poisons one element and puts it back"""
    g = torch.Generator().manual_seed(11)
    return {n: (torch.randn(n, generator=g) * 0.01).to(dev) for n in NORM_SIZES}


@contextlib.contextmanager
def _poisoned(buf, content):
    n = buf.numel()
    where = {"finite": None, "nan_first": (0, NAN), "nan_middle": (n // 2, NAN), "nan_last": (n - 1, NAN), "pos_inf": (n // 3, INF),
             "neg_inf": (n // 3, -INF), "big_3e19": (n // 2, 3e19)}[content]
    if where is None:
        yield
        return
    keep = buf[where[0]].clone()
    buf[where[0]] = where[1]
    try:
        yield
    finally:
        buf[where[0]] = keep


def _guarded_norm(ops, buf, scale, max_norm, guard, limit, loss=None, sentinel=-7.0):
    out = torch.full((2,), sentinel, dtype=torch.float32, device=buf.device)
    ops.grad_norm(buf, scale, max_norm, out, guard=guard, limit=limit, loss=loss)
    return out


@pytest.mark.parametrize("n", NORM_SIZES)
def test_finalize_every_content(dev, norm_buffers, n):
    """apply as the numpy model decides it, {total_norm, coef} the bits of the unguarded finalize, and without a max_norm no coef"""
    from drakegpt_amd import ops
    buf = norm_buffers[n]
    max_norm = torch.tensor([0.5], dtype=torch.float32, device=dev)
    limit = torch.tensor([GM.FLT_MAX], dtype=torch.float32, device=dev)
    for content in CONTENTS:
        with _poisoned(buf, content):
            want = ops.grad_norm(buf, 0.5, max_norm, torch.zeros(2, dtype=torch.float32, device=dev))
            guard = ops.new_update_guard(dev)
            got = _guarded_norm(ops, buf, 0.5, max_norm, guard, limit)
            bare = _guarded_norm(ops, buf, 0.5, None, ops.new_update_guard(dev), limit)
            host = buf.cpu().numpy()
        assert _same(got, want), (n, content, got.tolist(), want.tolist())
        assert _same(bare[:1], want[:1]) and bare[1].item() == -7.0, (n, content, bare.tolist())
        apply = GM.decide(want[0].item(), GM.FLT_MAX)
        assert apply == int(content == "finite"), (n, content, want.tolist())
        assert GM.reads_nonfinite(host) == (content != "finite"), (n, content)          # 3e19 included: the fp32-square caveat
        assert guard.tolist() == GM.advance([1, 0, 0, 0], apply), (n, content, guard.tolist())
    assert bool(torch.isfinite(buf).all())


@pytest.mark.parametrize("n", NORM_SIZES)
def test_finalize_counters_over_a_sequence(dev, norm_buffers, n):
    from drakegpt_amd import ops
    buf = norm_buffers[n]
    limit = torch.tensor([GM.FLT_MAX], dtype=torch.float32, device=dev)
    guard = ops.new_update_guard(dev)
    model = [1, 0, 0, 0]
    for k, content in enumerate(("finite", "nan_last", "pos_inf", "finite", "big_3e19", "neg_inf")):
        with _poisoned(buf, content):
            out = _guarded_norm(ops, buf, 1.0, None, guard, limit)
        model = GM.advance(model, GM.decide(out[0].item(), GM.FLT_MAX))
        assert guard.tolist() == model, (n, k, content, guard.tolist(), model)
    assert model == [0, 4, 2, 0]


def test_finalize_limit_and_loss(dev, norm_buffers):
    """a norm exactly equal to the limit applies, a limit one ulp below skips; a non-finite loss skips a clean gradient"""
    from drakegpt_amd import ops
    buf = norm_buffers[4099]
    out = ops.grad_norm(buf, 1.0, torch.ones(1, device=dev), torch.zeros(2, dtype=torch.float32, device=dev))
    t = np.float32(out[0].item())
    assert np.isfinite(t) and t > 0
    guard = ops.new_update_guard(dev)
    below = np.nextafter(t, np.float32(0))
    for lim, loss, want in ((t, None, 1), (below, None, 0), (np.nextafter(t, np.float32(np.inf)), None, 1), (t, 2.5, 1), (t, NAN, 0),
                            (t, INF, 0), (t, -INF, 0), (below, 2.5, 0)):
        limit = torch.tensor([lim], dtype=torch.float32, device=dev)
        loss_t = None if loss is None else torch.tensor(loss, dtype=torch.float32, device=dev)
        before = guard.tolist()
        got = _guarded_norm(ops, buf, 1.0, None, guard, limit, loss=loss_t)
        assert np.float32(got[0].item()) == t
        assert want == GM.decide(t, lim, loss)
        assert guard.tolist() == GM.advance(before, want), (lim, loss, guard.tolist())
    with pytest.raises(ValueError, match="guard needs limit"):
        ops.grad_norm(buf, 1.0, None, out, guard=guard)
    with pytest.raises(ValueError, match="go with guard"):
        ops.grad_norm(buf, 1.0, torch.ones(1, device=dev), out, limit=torch.ones(1, device=dev))


# ================================================================================================ AdamW
ADAMW_SIZES = (1, 4 * 256 * 3 + 3, 2048 * 1024 + 1024 + 5)
COMBOS = [(c, t, k, e) for c in (False, True) for t in (False, True) for k in (False, True) for e in (False, True)]


def _banded(n, dev, gen, dtype=torch.float32, scale=1.0, positive=False):
    """n values between two bands of BAND sentinels; returns (whole buffer, the view handed to the kernel)"""
    whole = torch.full((n + 2 * BAND,), 77.0, dtype=dtype, device=dev)
    vals = torch.randn(n, generator=gen) * scale
    whole[BAND:BAND + n] = (vals.abs() if positive else vals).to(dev, dtype)
    return whole, whole[BAND:BAND + n]


class _Case:
    """one set of banded buffers and operands per size; a combination (clip, table, mask, ema) selects what a launch is given"""

    def __init__(self, n, dev, seed=5):
        from drakegpt_amd import ops
        gen = torch.Generator().manual_seed(seed)
        self.n, self.dev = n, dev
        self.whole, self.view = {}, {}
        for name, kw in (("p", {}), ("g", dict(scale=0.1)), ("m", dict(scale=0.01)), ("v", dict(scale=1e-3, positive=True)), ("ema", {})):
            self.whole[name], self.view[name] = _banded(n, dev, gen, **kw)
        self.whole["shadow"], self.view["shadow"] = _banded(n, dev, gen, dtype=torch.bfloat16)
        self.hyper = torch.tensor([1e-3, 0.9, 0.95, 1e-8, 1e-2], dtype=torch.float32, device=dev)
        last = (n - 1) // 64 * 64
        self.clip = torch.tensor([0.625], dtype=torch.float32, device=dev)
        self.table = torch.tensor([1e-3, 5e-4, 2e-4], dtype=torch.float32, device=dev)
        self.bits = ops.new_no_decay_bits(sorted({(0, min(64, n)), (last, n)}), n, dev)
        self.ema_hyper = ops.new_ema_hyper(0.9, True, dev)
        self.state = ops.new_rng_state(3, dev, 1)          # step word 1: the table's second entry, the average's lerp branch
        self.data = ops.new_rng_state(9, dev, 40)

    def clone(self):
        import copy
        other = copy.copy(self)
        other.whole = {k: t.clone() for k, t in self.whole.items()}
        other.view = {k: other.whole[k][BAND:BAND + self.n] for k in self.whole}
        other.state, other.data = self.state.clone(), self.data.clone()
        return other

    def launch(self, ops, combo, **extra):
        v = self.view
        clip, table, mask, ema = combo
        kw = {}
        if clip:
            kw["clip"] = self.clip
        if table:
            kw["lr_table"] = self.table
        if mask:
            kw["no_decay_bits"] = self.bits
        if ema:
            kw.update(ema=v["ema"], ema_hyper=self.ema_hyper)
        ops.adamw_step(v["p"], v["g"], v["m"], v["v"], self.hyper, self.state, 0.5, shadow_bf16=v["shadow"], n=self.n, advance=True,
                       **kw, **extra)


@pytest.mark.parametrize("n", ADAMW_SIZES)
def test_adamw_guard_applied_is_the_unguarded_launch(dev, n):
    from drakegpt_amd import ops
    base = _Case(n, dev)
    for combo in COMBOS:
        ref, got, bare = base.clone(), base.clone(), base.clone()
        ref.launch(ops, combo)
        guard = ops.new_update_guard(dev)
        got.launch(ops, combo, guard=guard, data_state=got.data)
        for name in base.whole:
            assert _same(got.whole[name], ref.whole[name]), (n, combo, name)
        assert got.state.tolist() == ref.state.tolist() == [3, 0, 2, 0], (n, combo, got.state.tolist())
        assert got.data.tolist() == [9, 0, 41, 0] and guard.tolist() == [1, 0, 0, 0], (n, combo)
        # data_state absent: no word but the optimizer's moves
        bare.launch(ops, combo, guard=guard)
        assert bare.state.tolist() == [3, 0, 2, 0] and bare.data.tolist() == [9, 0, 40, 0], (n, combo)
        assert all(_same(bare.whole[name], ref.whole[name]) for name in base.whole), (n, combo)


@pytest.mark.parametrize("n", ADAMW_SIZES)
def test_adamw_guard_skipped_touches_nothing(dev, n):
    from drakegpt_amd import ops
    base = _Case(n, dev)
    for combo in COMBOS:
        ref, got = base.clone(), base.clone()
        ref.launch(ops, combo)
        clean = got.view["g"].clone()
        got.view["g"][n // 2] = NAN
        before = {k: t.clone() for k, t in got.whole.items()}
        guard = torch.tensor([0, 5, 2, 0], dtype=torch.int32, device=dev)
        got.launch(ops, combo, guard=guard, data_state=got.data)
        for name in base.whole:          # NaN gradient, sentinel bands and all
            assert _same(got.whole[name], before[name]), (n, combo, name)
        assert got.state.tolist() == [3, 0, 1, 0] and got.data.tolist() == [9, 0, 41, 0], (n, combo, got.state.tolist(), got.data.tolist())
        assert guard.tolist() == [0, 5, 2, 0]
        # a following applied launch gives what a first launch would have given
        got.view["g"].copy_(clean)
        guard[0:1].fill_(1)
        got.launch(ops, combo, guard=guard, data_state=got.data)
        for name in base.whole:
            assert _same(got.whole[name], ref.whole[name]), (n, combo, name)
        assert got.state.tolist() == [3, 0, 2, 0] and got.data.tolist() == [9, 0, 42, 0], (n, combo)
        bare = base.clone()
        guard[0:1].fill_(0)
        bare.launch(ops, combo, guard=guard)
        assert bare.state.tolist() == [3, 0, 1, 0] and bare.data.tolist() == [9, 0, 40, 0], (n, combo)
        assert all(_same(bare.whole[name], base.whole[name]) for name in base.whole), (n, combo)


def test_adamw_guard_argument_checks(dev):
    from drakegpt_amd import ops
    c = _Case(4, dev)
    combo = (False, False, False, False)
    with pytest.raises(ValueError, match="data_state goes with guard"):
        c.launch(ops, combo, data_state=c.data)
    with pytest.raises(ValueError, match="of its own"):
        c.launch(ops, combo, guard=ops.new_update_guard(dev), data_state=c.state)
    with pytest.raises(ValueError, match="4 words"):
        c.launch(ops, combo, guard=ops.new_update_guard(dev)[:2])


# ================================================================================================ engine
@pytest.fixture(scope="module")
def fix():
    """the tiny fixture model's initial weights, and five batches [16, 8] in which every token id occurs at most twice: this
    configuration sums the token-table gradient with fp32 atomics, whose order is free, and 0 + a + b is the same in either order --
    so two runs of the same program agree bit for bit and every comparison below is exact"""
    init = torch.load(os.path.join(GOLDEN, "traj5_TransformerLM.pt"), weights_only=True)["init"]
    g = torch.Generator().manual_seed(3)
    x = torch.stack([(torch.randperm(160, generator=g)[:128] % V).view(16, 8) for _ in range(5)])
    y = torch.stack([torch.randint(0, V, (16, 8), generator=g) for _ in range(5)])
    assert all(int(torch.bincount(b.flatten(), minlength=V).max()) <= 2 for b in x)
    return {"init": init, "x": x, "y": y}


def _engine(dev, fix, precision, graph, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0, precision=precision)
    m.load_state_dict(fix["init"])
    return TrainEngine(m.to(dev), 16, 8, lr=1e-3, betas=(0.9, 0.95), use_graph=graph, **kw)


def _feed(eng, fix, j, y=None):
    eng.set_batch(fix["x"][j][:16].to(eng.dev), (fix["y"][j][:16] if y is None else y).to(eng.dev))
    return eng.micro_step()


def _snap(eng):
    """the weights, both moments and every weight-derived copy (bf16 shadow, W^T, packed operands, moving average)"""
    torch.cuda.synchronize(eng.dev)
    out = {"flat": eng.flat[:eng.n_active], "m": eng.m_, "v": eng.v_, "wt": eng.wt_flat}
    for name in ("shadow", "ema", "wpack_flat", "shadow8", "wt8_flat"):
        if getattr(eng, name, None) is not None:
            out[name] = getattr(eng, name)
    return {k: t.clone() for k, t in out.items()}


def _assert_same_state(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert _same(a[k], b[k]), (what, k)


MODES = [("fp32", False), ("fp32", True), ("bf16", False), ("bf16", True)]
TABLE = [1e-3, 7e-4, 4e-4, 2e-4, 1e-4]
_REF = {}


def _reference(dev, fix, precision, graph, batches, **kw):
    """an engine WITHOUT the guard fed the given batches: (losses, state, step word), computed once per configuration"""
    key = (precision, graph, tuple(batches), tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _REF:
        eng = _engine(dev, fix, precision, graph, **kw)
        losses = [_feed(eng, fix, j).clone() for j in batches]
        _REF[key] = (losses, _snap(eng), eng.step_count())
    return _REF[key]


@pytest.mark.parametrize("precision,graph", MODES)
@pytest.mark.parametrize("kw", [dict(ema_decay=0.9), dict(max_grad_norm=0.05, ema_decay=0.9), dict(accum_steps=2)],
                         ids=["plain", "clip", "accum2"])
def test_engine_guard_on_and_nothing_skipped(dev, fix, precision, graph, kw):
    """(a) 4 steps with the guard on: the losses, weights, moments, derived copies and average of the engine without it"""
    want_losses, want, want_steps = _reference(dev, fix, precision, graph, (0, 1, 2, 3), **kw)
    eng = _engine(dev, fix, precision, graph, skip_nonfinite=True, skip_grad_norm=1e6, **kw)
    losses = [_feed(eng, fix, j).clone() for j in (0, 1, 2, 3)]
    _assert_same_state(_snap(eng), want, (precision, graph, kw))
    assert all(_same(a, b) for a, b in zip(losses, want_losses))
    assert eng.step_count() == want_steps and eng.micro_step_count() == 4 and eng.skipped_steps() == 0 and eng.consecutive_skips() == 0
    assert int(eng.last_step_applied) == 1 and float(eng.last_grad_norm) > 0
    if graph and kw.get("accum_steps", 1) == 1:
        assert len(eng._graphs) == 1


@pytest.mark.parametrize("precision,graph", MODES)
def test_engine_one_skipped_step(dev, fix, precision, graph):
    """(b) batches 0..3 with the limit below the norm at step 1: the engine without the guard fed 0, 2, 3 -- the table's entries
    0, 1, 2 included (another entry at any step would give other weights)"""
    kw = dict(lr_schedule=TABLE, ema_decay=0.9, ema_warmup=True)
    _, want, _ = _reference(dev, fix, precision, graph, (0, 2, 3), **kw)
    eng = _engine(dev, fix, precision, graph, skip_nonfinite=True, **kw)
    _feed(eng, fix, 0)
    before = _snap(eng)
    assert eng.current_lr() == np.float32(TABLE[1])
    eng.set_skip_grad_norm(1e-12)
    _feed(eng, fix, 1)
    eng.set_skip_grad_norm(None)
    _assert_same_state(_snap(eng), before, "the skipped step")
    assert int(eng.last_step_applied) == 0 and eng.step_count() == 1 and eng.micro_step_count() == 2 and eng.consecutive_skips() == 1
    assert eng.current_lr() == np.float32(TABLE[1])
    _feed(eng, fix, 2)
    _feed(eng, fix, 3)
    _assert_same_state(_snap(eng), want, (precision, graph))
    assert (eng.step_count(), eng.micro_step_count(), eng.skipped_steps(), eng.consecutive_skips()) == (3, 4, 1, 0)
    assert eng.current_lr() == np.float32(TABLE[3]) and eng.is_finite()


@pytest.mark.parametrize("precision,graph", MODES)
def test_engine_nonfinite_backward_is_skipped(dev, fix, precision, graph):
    """(c) an inf in one weight element makes the step's loss and gradient non-finite: nothing else moves, and with the element put
    back the run continues as the clean engine fed 0, 2, 3"""
    kw = dict(lr_schedule=TABLE, ema_decay=0.9, ema_warmup=True)
    _, want, _ = _reference(dev, fix, precision, graph, (0, 2, 3), **kw)
    eng = _engine(dev, fix, precision, graph, skip_nonfinite=True, **kw)
    _feed(eng, fix, 0)
    clean = _snap(eng)
    w = eng.param_view("1.w1")
    keep = w[3, 5].clone()
    w[3, 5] = INF
    eng.refresh_shadows()
    loss = _feed(eng, fix, 1)
    torch.cuda.synchronize(dev)
    assert not bool(torch.isfinite(loss)) or not bool(torch.isfinite(eng.last_grad_norm))
    assert int(eng.last_step_applied) == 0 and eng.step_count() == 1 and eng.micro_step_count() == 2
    assert bool(torch.isinf(w[3, 5]))
    w[3, 5] = keep
    eng.refresh_shadows()
    _assert_same_state(_snap(eng), clean, "after the poisoned step")
    _feed(eng, fix, 2)
    _feed(eng, fix, 3)
    _assert_same_state(_snap(eng), want, (precision, graph))
    assert (eng.step_count(), eng.skipped_steps(), eng.consecutive_skips()) == (3, 1, 0) and eng.is_finite()


@pytest.mark.parametrize("precision,graph", MODES)
def test_engine_poisoned_accumulator_skips_the_whole_step(dev, fix, precision, graph):
    """(c) accum_steps 2: a NaN written into gacc between the two micro-steps skips that optimizer step; the next one overwrites
    gacc at j == 0 and the run continues as the engine without the guard fed (0, 1), (4, 0)"""
    _, want, _ = _reference(dev, fix, precision, graph, (0, 1, 4, 0), accum_steps=2)
    eng = _engine(dev, fix, precision, graph, skip_nonfinite=True, accum_steps=2)
    _feed(eng, fix, 0)
    _feed(eng, fix, 1)
    clean = _snap(eng)
    _feed(eng, fix, 2)
    eng.gacc[eng.n_active // 2] = NAN
    _feed(eng, fix, 3)
    _assert_same_state(_snap(eng), clean, "the skipped optimizer step")
    assert int(eng.last_step_applied) == 0 and eng.step_count() == 1 and eng.micro_step_count() == 4
    _feed(eng, fix, 4)
    _feed(eng, fix, 0)
    _assert_same_state(_snap(eng), want, (precision, graph))
    assert (eng.step_count(), eng.micro_step_count(), eng.skipped_steps(), eng.consecutive_skips()) == (2, 6, 1, 0)


def test_engine_without_the_guard_is_lost(dev, fix):
    """(d) the contrast: the same poison, no guard -- every weight and both moments are gone after one step"""
    eng = _engine(dev, fix, "fp32", True)
    _feed(eng, fix, 0)
    assert eng.is_finite() and eng.last_step_applied is None
    eng.param_view("1.w1")[3, 5] = INF
    eng.refresh_shadows()
    _feed(eng, fix, 1)
    assert not eng.is_finite()
    for call in (eng.skipped_steps, eng.consecutive_skips, lambda: eng.set_skip_grad_norm(1.0)):
        with pytest.raises(RuntimeError, match="without the update guard"):
            call()


@pytest.mark.parametrize("graph", [False, True])
def test_engine_every_target_ignored(dev, fix, graph):
    """(e) ignore_index with no target left: a NaN loss over a zero gradient.  The norm is 0, so the loss operand alone skips the
    step -- the weights keep their bits (no weight decay either)"""
    eng = _engine(dev, fix, "fp32", graph, skip_nonfinite=True, ignore_index=-100, weight_decay=0.1)
    _feed(eng, fix, 0)
    before = _snap(eng)
    loss = _feed(eng, fix, 1, y=torch.full((16, 8), -100, dtype=torch.int64))
    _assert_same_state(_snap(eng), before, "all ignored")
    assert bool(torch.isnan(loss)) and float(eng.last_grad_norm) == 0.0 and int(eng.last_step_applied) == 0
    assert (eng.step_count(), eng.micro_step_count(), eng.skipped_steps()) == (1, 2, 1)
    _feed(eng, fix, 2)
    assert (eng.step_count(), eng.consecutive_skips()) == (2, 0) and eng.is_finite()


# ---- (f) launch accounting: the recorder of tests/test_gpu_step_launches.py, restated
@contextlib.contextmanager
def _recording(calls):
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


def _trace(dev, fix, **kw):
    eng = _engine(dev, fix, "fp32", False, **kw)
    calls = []
    with _recording(calls):
        _feed(eng, fix, 0)
    torch.cuda.synchronize(dev)
    return calls


def test_engine_launch_accounting(dev, fix):
    default, clip = _trace(dev, fix), _trace(dev, fix, max_grad_norm=1.0)
    guard, both = _trace(dev, fix, skip_nonfinite=True), _trace(dev, fix, skip_nonfinite=True, max_grad_norm=1.0)
    i = default.index("dg_adamw_step")
    assert default.count("dg_adamw_step") == 1
    assert guard == default[:i] + ["dg_sumsq_partials", "dg_grad_norm_finalize_guard", "dg_adamw_step_guard"] + default[i + 1:]
    swap = {"dg_grad_norm_finalize": "dg_grad_norm_finalize_guard", "dg_adamw_step_clip": "dg_adamw_step_guard"}
    assert both == [swap.get(c, c) for c in clip] and len(both) == len(clip) and both != clip
    assert not any("guard" in c for c in default + clip)
    eng = _engine(dev, fix, "fp32", True, skip_nonfinite=True)
    _feed(eng, fix, 0)
    torch.cuda.synchronize(dev)
    assert len(eng._graphs) == 1


# ---- (g) resume
@pytest.mark.parametrize("precision,graph", [("fp32", False), ("bf16", True)])
def test_engine_resume_after_a_skipped_step(dev, fix, precision, graph):
    kw = dict(lr_schedule=TABLE, ema_decay=0.9, skip_grad_norm=1e6)
    a = _engine(dev, fix, precision, graph, **kw)
    _feed(a, fix, 0)
    a.set_skip_grad_norm(1e-12)
    _feed(a, fix, 1)
    a.set_skip_grad_norm(2e6)
    sd = a.state_dict()
    assert sd["meta"]["update_guard"] is True
    assert sd["engine"]["guard"] == {"skipped": 1, "consecutive": 1, "limit": 2e6, "opt_step": 1} and sd["engine"]["step_word"] == 2
    _feed(a, fix, 2)
    _feed(a, fix, 3)
    b = _engine(dev, fix, precision, graph, skip_nonfinite=True, lr_schedule=TABLE, ema_decay=0.9)
    b.load_state_dict(sd)
    assert (b.step_count(), b.micro_step_count(), b.skipped_steps(), b.consecutive_skips()) == (1, 2, 1, 1)
    assert b.skip_grad_norm == 2e6 and b.guard_limit.item() == np.float32(2e6) and int(b.last_step_applied) == 0
    _feed(b, fix, 2)
    _feed(b, fix, 3)
    _assert_same_state(_snap(b), _snap(a), (precision, graph))
    for e in (a, b):
        assert (e.step_count(), e.micro_step_count(), e.skipped_steps(), e.consecutive_skips()) == (3, 4, 1, 0)
    # a guarded file into an engine without the guard: refused, naming the field
    plain = _engine(dev, fix, precision, graph, lr_schedule=TABLE, ema_decay=0.9)
    with pytest.raises(ValueError, match=r"meta\.update_guard differs"):
        plain.load_state_dict(sd)
    # an unguarded file into a guarded engine: accepted, the optimizer word starts at the step word, the counters at 0
    _feed(plain, fix, 0)
    _feed(plain, fix, 1)
    old = plain.state_dict()
    assert "guard" not in old["engine"] and "update_guard" not in old["meta"]
    c = _engine(dev, fix, precision, graph, skip_grad_norm=5.0, lr_schedule=TABLE, ema_decay=0.9)
    c.load_state_dict(old)
    assert (c.step_count(), c.micro_step_count(), c.skipped_steps(), c.consecutive_skips()) == (2, 2, 0, 0) and c.skip_grad_norm == 5.0
    _feed(plain, fix, 2)
    c.set_skip_grad_norm(None)
    _feed(c, fix, 2)
    _assert_same_state(_snap(c), _snap(plain), "guard turned on mid-run")


# ---- (h) the scaled preset at B 16
@contextlib.contextmanager
def _one_rank_group():
    import torch.distributed as dist
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "store"), rank=0, world_size=1)
        try:
            yield dist.group.WORLD
        finally:
            dist.destroy_process_group()


def _scaled(dev, precision, dp=False, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.config import PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = PRESETS["scaled"]
    T = cfg["context_length"]
    torch.manual_seed(42)
    m = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=precision).to(dev)
    eng = TrainEngine(m, 16, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=7, use_graph=True, **kw)
    eng.force_dp_path = dp
    eng.set_corpus(torch.randint(0, V, (20_000,), generator=torch.Generator().manual_seed(1)))
    eng.stage_offsets(torch.randint(20_000 - T - 1, (4, 16), generator=torch.Generator().manual_seed(2)))
    losses = [eng.step().clone() for _ in range(2)]
    eng.check_status()
    return eng, losses


def test_scaled_bf16_three_buckets_one_rank_group(dev):
    with _one_rank_group() as pg:
        off, off_losses = _scaled(dev, "bf16", dp=True, process_group=pg, dp_buckets=3)
        on, on_losses = _scaled(dev, "bf16", dp=True, process_group=pg, dp_buckets=3, skip_nonfinite=True)
        assert on.dp_buckets == 3
        _assert_same_state(_snap(on), _snap(off), "scaled bf16, 3 buckets")
        assert all(_same(a, b) for a, b in zip(on_losses, off_losses))
        assert (on.step_count(), on.micro_step_count(), on.skipped_steps()) == (2, 2, 0)


def test_scaled_fp8(dev):
    off, off_losses = _scaled(dev, "fp8")
    on, on_losses = _scaled(dev, "fp8", skip_grad_norm=1e6)
    _assert_same_state(_snap(on), _snap(off), "scaled fp8")
    assert all(_same(a, b) for a, b in zip(on_losses, off_losses))
    assert sorted(on.fp8_sites) == sorted(off.fp8_sites) and all(_same(on.fp8_sites[k], off.fp8_sites[k]) for k in on.fp8_sites)
    assert (on.step_count(), on.micro_step_count(), on.skipped_steps()) == (2, 2, 0)


# ================================================================================================ optim.AdamW
def _two_groups(dev, **kw):
    from drakegpt_amd import optim
    torch.manual_seed(3)
    a, b = torch.nn.Linear(37, 19).to(dev), torch.nn.Linear(19, 5).to(dev)
    opt = optim.AdamW([{"params": list(a.parameters())}, {"params": list(b.parameters()), "weight_decay": 0.0}], lr=1e-2, **kw)
    return list(a.parameters()) + list(b.parameters()), opt


def _set_grads(params, k, poison=False):
    g = torch.Generator().manual_seed(100 + k)
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * 0.1).to(p.device)
    if poison:
        params[-1].grad[2] = NAN          # the second group's bias


def _optim_state(params, opt):
    torch.cuda.synchronize()
    out = {f"p{i}": p.detach().clone() for i, p in enumerate(params)}
    for gi, fl in opt._flat.items():
        out.update({f"m{gi}": fl.m.clone(), f"v{gi}": fl.v.clone(), f"t{gi}": fl.t.clone()})
        if fl.ema is not None:
            out[f"ema{gi}"] = fl.ema.clone()
    return out


@pytest.mark.parametrize("clip", [None, 0.05])
def test_optim_guard(dev, clip):
    kw = dict(ema_decay=0.9, **({} if clip is None else {"max_grad_norm": clip}))
    ref_p, ref = _two_groups(dev, **kw)
    got_p, got = _two_groups(dev, skip_nonfinite=True, **kw)
    assert got.last_step_applied is None
    for k in (0, 1):
        for ps, opt in ((ref_p, ref), (got_p, got)):
            _set_grads(ps, k)
            opt.step()
    _assert_same_state(_optim_state(got_p, got), _optim_state(ref_p, ref), ("no skip", clip))
    assert int(got.last_step_applied) == 1 and got.skipped_steps() == 0 and float(got.last_grad_norm) > 0
    # a NaN in the second group's gradient: neither group moves, neither t moves
    before = _optim_state(got_p, got)
    _set_grads(got_p, 7, poison=True)
    got.step()
    _assert_same_state(_optim_state(got_p, got), before, ("skipped", clip))
    assert int(got.last_step_applied) == 0 and got.skipped_steps() == 1 and got.consecutive_skips() == 1
    assert [fl.t[2].item() for fl in got._flat.values()] == [2, 2]
    sd = got.state_dict()
    assert sd["guard"] == {"skipped": 1, "consecutive": 1, "limit": None} and "guard" not in ref.state_dict()
    # the limit: below the norm skips, and the run then goes on as the unguarded optimizer's
    got.set_skip_grad_norm(1e-12)
    _set_grads(got_p, 2)
    got.step()
    _assert_same_state(_optim_state(got_p, got), before, ("limit", clip))
    assert got.skipped_steps() == 2 and got.consecutive_skips() == 2
    got.set_skip_grad_norm(None)
    for ps, opt in ((ref_p, ref), (got_p, got)):
        _set_grads(ps, 2)
        opt.step()
    _assert_same_state(_optim_state(got_p, got), _optim_state(ref_p, ref), ("after the skips", clip))
    assert got.consecutive_skips() == 0 and got.is_finite()
    # the contrast: the unguarded optimizer takes the NaN
    _set_grads(ref_p, 7, poison=True)
    ref.step()
    assert not ref.is_finite()


# ================================================================================================ harness
def _eval_lines(out):
    return [json.loads(s) for s in out.splitlines() if s.startswith("{") and '"val_loss"' in s]


@pytest.mark.parametrize("model", ["TransformerLM", "BlocksLM"])
def test_train_harness(dev, capsys, monkeypatch, model):
    from drakegpt_amd import train
    base = ["--model", model, "--iters", "6", "--eval-interval", "2", "--eval-iters", "2", "--precision", "fp32", "--no-save", "--sample", "3"]
    built = {}
    real = train.build_model

    def keeping(*a, **kw):
        out = real(*a, **kw)
        built["model"] = out[0]
        built["init"] = {k: v.detach().clone() for k, v in out[0].state_dict().items()}
        return out
    monkeypatch.setattr(train, "build_model", keeping)
    with pytest.raises(RuntimeError, match="skipped 4 optimizer updates in a row"):
        train.main(base + ["--skip-nonfinite", "--skip-grad-norm", "1e-9", "--max-consecutive-skips", "3"])
    lines = _eval_lines(capsys.readouterr().out)
    assert [ln["step"] for ln in lines] == [2] and lines[0]["skipped"] == 2
    now = built["model"].state_dict()
    assert now.keys() == built["init"].keys() and all(_same(now[k], built["init"][k]) for k in now)
    train.main(base + ["--skip-nonfinite", "--skip-grad-norm", "1e9"])
    lines = _eval_lines(capsys.readouterr().out)
    assert [ln["step"] for ln in lines] == [2, 4, 6] and all(ln["skipped"] == 0 for ln in lines)
    train.main(base)
    lines = _eval_lines(capsys.readouterr().out)
    assert len(lines) == 3 and not any("skipped" in ln for ln in lines)
