"""CPU: the host side of gradient accumulation -- the numpy restatement of dg_grad_accumulate (tests/accum_model.py) on hand-made
sequences, check_accum_steps, the harness flag, and engine_loop(accum_steps=K): K blocks of offsets per optimizer step, drawn in
the order a loop of K get_batch calls would, never staged across an evaluation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import accum_model as AM  # noqa: E402

from drakegpt_amd import preprocessing, train  # noqa: E402
from drakegpt_amd.optim import check_accum_steps  # noqa: E402


def test_model_sums_in_call_order_and_cycles():
    rng = np.random.default_rng(0)
    for k in (1, 2, 3):
        m = AM.AccumModel(7, k, step=5, scratch=9)
        m.acc[:] = np.nan                                   # j == 0 overwrites: whatever the accumulator held is gone
        gs, ls = [], []
        for c in range(2 * k + 1):
            g = rng.standard_normal(7).astype(np.float32)
            l = np.float32(rng.random())
            gs.append(g); ls.append(l)
            m.call(g, l)
            j = c % k
            want = gs[c - j].copy()
            s = np.float32(ls[c - j])
            for i in range(c - j + 1, c + 1):
                want = want + gs[i]
                s = np.float32(s + ls[i])
            assert want.dtype == np.float32 and np.array_equal(m.acc, want)
            assert m.ctl.tolist() == [(c + 1) % k, k, 0, 0]
            assert m.rng_state.tolist() == [0, 0, 5 + c + 1, 9]
            assert m.loss_out[0] == s
            if j == k - 1:
                assert m.loss_out[1] == np.float32(s / np.float32(k))


def test_model_step_word_wraps():
    m = AM.AccumModel(1, 2, step=0xFFFFFFFF)
    m.call(np.ones(1, np.float32))
    assert int(m.rng_state[2]) == 0


def test_check_accum_steps():
    for ok in (1, 2, 64):
        assert check_accum_steps(ok) == ok
    for bad in (0, -1, True, False, 2.0, 1.5, "2", None, float("nan")):
        with pytest.raises(ValueError):
            check_accum_steps(bad)


def test_train_parser_has_accum_steps():
    p = train.build_parser()
    assert p.parse_args([]).accum_steps == 1
    assert p.parse_args(["--accum-steps", "4"]).accum_steps == 4
    with pytest.raises(SystemExit):
        p.parse_args(["--accum-steps", "2.5"])


@pytest.mark.parametrize("iters,interval,world", [(6, 2, 1), (7, 3, 2), (4, 10, 1)])
def test_engine_loop_draws_K_blocks_per_optimizer_step(iters, interval, world):
    n_train, T, B, eval_iters, K = 5000, 8, 4, 3, 3

    class FakeEngine:
        def __init__(self):
            self.seen, self.block, self.at, self.stages, self.evals_at_stage = [], None, 0, [], []

        def stage_offsets(self, block):
            assert block.dim() == 2 and block.shape[1] == B
            assert block.shape[0] % K == 0                       # TrainEngine.stage_offsets demands it
            assert self.block is None or self.at == self.block.shape[0]      # the previous stage is used up
            self.stages.append(block.shape[0])
            self.evals_at_stage.append(len(ev))
            self.block, self.at = block.clone(), 0

        def step(self):                                          # one optimizer step: the next K rows
            for _ in range(K):
                self.seen.append(self.block[self.at])
                self.at += 1

        def check_status(self):
            self.checked = True

    def eval_draws(gen, sink):
        for _ in range(2 * eval_iters):
            sink.append(preprocessing.draw_offsets(n_train, T, B, gen))

    for rank in range(world):
        gen = torch.Generator().manual_seed(42)
        ev = []
        eng = FakeEngine()
        train.engine_loop(eng, n_train, T, B, rank, world, iters, interval, lambda it: eval_draws(gen, ev), "cpu", generator=gen,
                          accum_steps=K)
        gen2 = torch.Generator().manual_seed(42)
        want, ev2 = [], []
        for it in range(iters):
            for _ in range(K):                                   # a loop of K get_batch calls per iteration
                ix = torch.randint(n_train - T, (B * world,), generator=gen2)
                want.append(ix[rank * B:(rank + 1) * B])
            if (it + 1) % interval == 0:
                eval_draws(gen2, ev2)
        assert len(eng.seen) == iters * K and all(torch.equal(a, b) for a, b in zip(eng.seen, want)) and eng.checked
        assert len(ev) == len(ev2) and all(torch.equal(a, b) for a, b in zip(ev, ev2))
        assert torch.equal(torch.randint(100, (4,), generator=gen), torch.randint(100, (4,), generator=gen2))
        # one stage per evaluation interval, K rows per optimizer step, staged right after the previous interval's evaluation
        n_stage = (iters + interval - 1) // interval
        assert eng.stages == [K * min(interval, iters - s * interval) for s in range(n_stage)]
        assert eng.evals_at_stage == [s * 2 * eval_iters for s in range(n_stage)]


def test_engine_loop_default_is_one_block_per_step():
    """the trailing keyword defaults to 1: existing positional call sites draw what they always drew"""
    n_train, T, B = 5000, 8, 4
    rows = []

    class FakeEngine:
        def stage_offsets(self, block):
            rows.append(block.shape[0])

        def step(self):
            pass

        def check_status(self):
            pass

    train.engine_loop(FakeEngine(), n_train, T, B, 0, 1, 5, 2, lambda it: None, "cpu", torch.Generator().manual_seed(1))
    assert rows == [2, 2, 1]
