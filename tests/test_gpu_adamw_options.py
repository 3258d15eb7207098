"""All 32 AdamW kernels (clip x LR table x no-decay bitmap x moving average x update guard), each through the entry ops.adamw_step
routes it to, against the plain entries of the same library on the same device.  Every comparison is bitwise: no tolerance.

  neutral   coefficient 1.0, a table whose every entry is hyper[0], an all-zero bitmap, guard word 1: p, m, v, the shadow and the four
            state words of plain dg_adamw_step on the same inputs (include/drakegpt_hip.h promises each of these singly)
  live      a coefficient != 1, a 3-entry table read at step words 0 / 1 / 7, a bitmap with isolated bits, a live average: whatever goes
            through dg_adamw_step_ema or dg_adamw_step_guard gives dg_adamw_step_sched's p / m / v / shadow / state for the same clip /
            table / bitmap, and the average of tests/ema_model.py
  skipped   guard word 0: every buffer keeps its bytes, the optimizer's step word stays, the arrival word is 0, and a data_state's
            step word moves on

Sizes: a tail alone; 16 vectors and a tail; the bitmap's second word; the grid cap, a second grid-stride trip and a tail.  Each with a
bf16 shadow that is 8-byte aligned (one store per lane) and one that is a single element off (scalar stores)."""
import contextlib
import copy
import itertools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_model as EM  # noqa: E402

pytestmark = pytest.mark.gpu
N_BIG = 2048 * 256 * 4 + 64 * 5 + 3
SIZES = (3, 67, 2117, N_BIG)
BAND = 64                       # sentinels on either side of every buffer (64 floats: the views stay 16-byte aligned)
HYPER = [1e-3, 0.9, 0.95, 1e-8, 1e-2]
SCALE = 0.5
DECAY, WARMUP = 0.9, True
FLAGS = list(itertools.product((False, True), repeat=3))                     # (clip, table, bitmap)
COMBOS = [f + (e, gd) for gd in (False, True) for e in (False, True) for f in FLAGS]
NAMES = ("p", "g", "m", "v", "ema", "shadow")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class _Buffers:
    """p, g, m, v, ema and the shadow between two bands of sentinels, the state words, and the operands of either flavour"""

    def __init__(self, n, shadow_off, dev):
        from drakegpt_amd import ops
        gen = torch.Generator().manual_seed(1000 + n)
        self.n, self.off, self.dev = n, shadow_off, dev
        self.whole = {}
        for name, scale, positive in (("p", 1.0, False), ("g", 0.1, False), ("m", 0.01, False), ("v", 1e-3, True), ("ema", 1.0, False)):
            vals = torch.randn(n, generator=gen) * scale
            self.whole[name] = torch.full((n + 2 * BAND,), 77.0, dtype=torch.float32, device=dev)
            self.whole[name][BAND:BAND + n] = (vals.abs() if positive else vals).to(dev)
        self.whole["shadow"] = torch.full((n + 2 * BAND + 1,), 77.0, dtype=torch.bfloat16, device=dev)
        self.state = ops.new_rng_state(3, dev, 1)
        self.data = ops.new_rng_state(9, dev, 40)

    def view(self, name):
        lo = BAND + (self.off if name == "shadow" else 0)
        return self.whole[name][lo:lo + self.n]

    def clone(self, step=None):
        other = copy.copy(self)
        other.whole = {k: t.clone() for k, t in self.whole.items()}
        other.state, other.data = self.state.clone(), self.data.clone()
        if step is not None:
            other.state[2] = step
        return other


class _Operands:
    def __init__(self, n, dev, live):
        from drakegpt_amd import ops
        self.hyper = torch.tensor(HYPER, dtype=torch.float32, device=dev)
        self.ema_hyper = ops.new_ema_hyper(DECAY, WARMUP, dev)
        if live:
            last = (n - 1) // 64 * 64                                                      # the last granule, whole or not
            ranges = {(0, min(64, n)), (last, n)} | ({(128, 192)} if n > 192 else set()) | ({(2048, 2112)} if n > 2112 else set())
            self.clip = torch.tensor([0.625], dtype=torch.float32, device=dev)
            self.table = torch.tensor([1e-3, 5e-4, 2e-4], dtype=torch.float32, device=dev)
            self.bits = ops.new_no_decay_bits(sorted(ranges), n, dev)
        else:
            self.clip = torch.ones(1, dtype=torch.float32, device=dev)
            self.table = torch.tensor([HYPER[0]] * 3, dtype=torch.float32, device=dev)
            self.bits = ops.new_no_decay_bits([], n, dev)

    def pick(self, flags):
        clip, table, bitmap = flags
        return (self.clip if clip else None, self.table if table else None, self.bits if bitmap else None)


def _routed(ops, b, o, combo, guard=None, data_state=None, advance=True):
    """ops.adamw_step with what the combination names: the entry is the wrapper's choice"""
    clip, table, bits = o.pick(combo[:3])
    kw = {}
    if combo[3]:
        kw.update(ema=b.view("ema"), ema_hyper=o.ema_hyper)
    if combo[4]:
        kw.update(guard=guard, data_state=data_state)
    ops.adamw_step(b.view("p"), b.view("g"), b.view("m"), b.view("v"), o.hyper, b.state, SCALE, shadow_bf16=b.view("shadow"), n=b.n,
                   advance=advance, clip=clip, lr_table=table, no_decay_bits=bits, **kw)


def _plain(ops, b, o):
    ops.check(ops.lib.dg_adamw_step(ops._p(b.view("p")), ops._p(b.view("g")), ops._p(b.view("m")), ops._p(b.view("v")), b.n, ops._p(o.hyper),
                                    ops._p(b.state), SCALE, ops._p(b.view("shadow")), 1, ops._stream()), "dg_adamw_step")


def _sched(ops, b, o, flags):
    clip, table, bits = o.pick(flags)
    ops.check(ops.lib.dg_adamw_step_sched(ops._p(b.view("p")), ops._p(b.view("g")), ops._p(b.view("m")), ops._p(b.view("v")), b.n,
                                          ops._p(o.hyper), ops._p(b.state), SCALE, ops._p(clip), ops._p(table),
                                          0 if table is None else table.numel(), ops._p(bits), ops._p(b.view("shadow")), 1, ops._stream()),
              "dg_adamw_step_sched")


@pytest.fixture(scope="module", params=[(n, off) for n in SIZES for off in (0, 1)], ids=lambda c: f"n{c[0]}-shadow+{c[1]}")
def base(request, dev):
    n, off = request.param
    b = _Buffers(n, off, dev)
    assert b.view("p").data_ptr() % 16 == 0 and b.view("ema").data_ptr() % 16 == 0
    assert b.view("shadow").data_ptr() % 8 == 2 * off
    return b


@contextlib.contextmanager
def _recording(ops, calls):
    """appends the `what` of every ops.check to calls"""
    check = ops.check

    def counting(rc, what):
        calls.append(what)
        return check(rc, what)
    ops.check = counting
    try:
        yield
    finally:
        ops.check = check


def test_every_combination_reaches_its_entry(dev):
    from drakegpt_amd import ops
    b, o = _Buffers(67, 0, dev), _Operands(67, dev, live=True)
    for combo in COMBOS:
        clip, table, bitmap, ema, gd = combo
        want = ("dg_adamw_step_guard" if gd else "dg_adamw_step_ema" if ema else "dg_adamw_step_sched" if table or bitmap else
                "dg_adamw_step_clip" if clip else "dg_adamw_step")
        calls = []
        with _recording(ops, calls):
            _routed(ops, b.clone(), o, combo, guard=ops.new_update_guard(dev))
        assert calls == [want], (combo, calls)
    torch.cuda.synchronize()


def test_neutral_options_give_the_plain_step(dev, base):
    from drakegpt_amd import ops
    o = _Operands(base.n, dev, live=False)
    want = base.clone()
    _plain(ops, want, o)
    assert want.state.tolist() == [3, 0, 2, 0]
    assert not _same(want.whole["p"], base.whole["p"]) and _same(want.whole["ema"], base.whole["ema"])
    for combo in COMBOS:
        got = base.clone()
        guard = ops.new_update_guard(dev)
        _routed(ops, got, o, combo, guard=guard, data_state=got.data)
        for name in ("p", "g", "m", "v", "shadow"):
            assert _same(got.whole[name], want.whole[name]), (base.n, base.off, combo, name)
        assert got.state.tolist() == want.state.tolist(), (combo, got.state.tolist())
        assert got.data.tolist() == ([9, 0, 41, 0] if combo[4] else [9, 0, 40, 0]) and guard.tolist() == [1, 0, 0, 0], combo
        if not combo[3]:
            assert _same(got.whole["ema"], base.whole["ema"]), combo


@pytest.mark.parametrize("step", [0, 1, 7])
def test_live_options_against_the_sched_entry_and_the_ema_model(dev, base, step):
    from drakegpt_amd import ops
    o = _Operands(base.n, dev, live=True)
    start = base.clone(step)
    refs, averages = {}, {}
    for flags in FLAGS:
        refs[flags] = start.clone()
        _sched(ops, refs[flags], o, flags)
        assert refs[flags].state.tolist() == [3, 0, step + 1, 0]
    # the options are live: the table, the bitmap and the coefficient each change the weights
    if step != 0:
        assert not _same(refs[(False, True, False)].whole["p"], refs[(False, False, False)].whole["p"])
    assert not _same(refs[(False, False, True)].whole["p"], refs[(False, False, False)].whole["p"])
    assert not _same(refs[(True, False, False)].whole["p"], refs[(False, False, False)].whole["p"])
    for combo in COMBOS:
        if not (combo[3] or combo[4]):
            continue
        want, got = refs[combo[:3]], start.clone()
        guard = ops.new_update_guard(dev)
        _routed(ops, got, o, combo, guard=guard, data_state=got.data)
        for name in ("p", "g", "m", "v", "shadow"):
            assert _same(got.whole[name], want.whole[name]), (base.n, base.off, step, combo, name)
        assert got.state.tolist() == want.state.tolist(), (combo, got.state.tolist())
        if not combo[3]:
            assert _same(got.whole["ema"], start.whole["ema"]), combo
            continue
        if combo[:3] not in averages:
            model = EM.step(start.view("ema").cpu().numpy(), want.view("p").cpu().numpy(), DECAY, WARMUP, step)
            averages[combo[:3]] = start.whole["ema"].clone()
            averages[combo[:3]][BAND:BAND + base.n] = torch.from_numpy(model).to(dev)
        assert _same(got.whole["ema"], averages[combo[:3]]), (base.n, base.off, step, combo)
        if step == 0:
            assert _same(got.view("ema"), got.view("p"))


def test_guard_word_zero_touches_nothing(dev, base):
    from drakegpt_amd import ops
    o = _Operands(base.n, dev, live=True)
    for combo in COMBOS:
        if not combo[4]:
            continue
        for with_data, advance in ((True, True), (False, True), (True, False)):
            got = base.clone()
            guard = torch.tensor([0, 5, 2, 0], dtype=torch.int32, device=dev)
            _routed(ops, got, o, combo, guard=guard, data_state=got.data if with_data else None, advance=advance)
            for name in NAMES:
                assert _same(got.whole[name], base.whole[name]), (base.n, base.off, combo, name)
            assert got.state.tolist() == [3, 0, 1, 0], (combo, got.state.tolist())
            assert got.data.tolist() == [9, 0, 41 if with_data and advance else 40, 0], (combo, with_data, advance, got.data.tolist())
            assert guard.tolist() == [0, 5, 2, 0]
