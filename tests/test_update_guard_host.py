"""CPU: the update guard's decision rule and counters (tests/guard_model.py), its option checks, the state-format rules in all three
load directions on hand-built dicts, and the harness flags -- everything of the feature that runs without a GPU."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_model as GM  # noqa: E402


def test_decision_rule():
    inf, nan = float("inf"), float("nan")
    assert GM.decide(1.0, GM.FLT_MAX) == 1 and GM.decide(GM.FLT_MAX, GM.FLT_MAX) == 1
    assert GM.decide(inf, GM.FLT_MAX) == 0 and GM.decide(nan, GM.FLT_MAX) == 0
    assert GM.decide(inf, inf) == 1          # why the staged limit is FLT_MAX, never +inf
    assert GM.decide(2.0, 2.0) == 1 and GM.decide(2.0, np.nextafter(np.float32(2.0), np.float32(0.0))) == 0
    assert GM.decide(1.0, 2.0, loss=3.5) == 1
    for bad in (inf, -inf, nan):
        assert GM.decide(1.0, 2.0, loss=bad) == 0
    assert GM.decide(3.0, 2.0, loss=1.0) == 0


def test_counters():
    final, trace = GM.run([1, 0, 0, 1, 0, 1])
    assert trace == [[1, 0, 0, 0], [0, 1, 1, 0], [0, 2, 2, 0], [1, 2, 0, 0], [0, 3, 1, 0], [1, 3, 0, 0]] and final == trace[-1]
    assert GM.run([0] * 5)[0] == [0, 5, 5, 0]
    assert GM.run([1, 1], guard=(0, 7, 3, 0))[0] == [1, 7, 0, 0]
    assert GM.words([1, 0, 1, 1]) == (4, 3)


def test_fp32_square_caveat():
    assert not GM.reads_nonfinite([1.0, -2.0, 1.8e19])
    assert GM.reads_nonfinite([1.0, 3e19]) and GM.reads_nonfinite([-3e19])
    assert GM.reads_nonfinite([float("nan")]) and GM.reads_nonfinite([float("inf")]) and GM.reads_nonfinite([0.0, -float("inf")])


def test_check_guard_options():
    from drakegpt_amd import ops
    assert ops.check_guard_options() == (False, None) and ops.check_guard_options(False, None) == (False, None)
    assert ops.check_guard_options(True) == (True, GM.FLT_MAX) and ops.GUARD_NONFINITE_LIMIT == GM.FLT_MAX
    assert ops.check_guard_options(False, 2.5) == (True, 2.5)          # skip_grad_norm implies the non-finite guard
    assert ops.check_guard_options(True, 1e-9) == (True, 1e-9)
    on, lim = ops.check_guard_options(True, np.float32(0.5))
    assert on is True and isinstance(lim, float) and lim == 0.5
    assert ops.check_guard_options(True, 1e300) == (True, GM.FLT_MAX)          # (what fp32 can hold)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), True, False, "x", [1.0]):
        with pytest.raises(ValueError, match="skip_grad_norm"):
            ops.check_guard_options(True, bad)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            ops.check_guard_options(bad)
    g = ops.new_update_guard("cpu")
    assert g.dtype == torch.int32 and g.tolist() == [1, 0, 0, 0]


def test_layers_check_before_touching_a_device():
    from drakegpt_amd import optim
    lin = torch.nn.Linear(3, 3)
    for kw in (dict(skip_grad_norm=0.0), dict(skip_grad_norm=float("nan")), dict(skip_grad_norm=float("inf")), dict(skip_nonfinite=1),
               dict(skip_grad_norm=True)):
        with pytest.raises(ValueError, match="skip_"):
            optim.AdamW(lin.parameters(), **kw)
    opt = optim.AdamW(lin.parameters())
    assert opt.guard_on is False and "guard" not in opt.state_dict() and opt.last_step_applied is None
    for call in (opt.skipped_steps, opt.consecutive_skips, lambda: opt.set_skip_grad_norm(1.0)):
        with pytest.raises(RuntimeError, match="without the update guard"):
            call()
    with pytest.raises(ValueError, match="guard differs"):
        opt.load_state_dict(dict(opt.state_dict(), guard={"skipped": 1, "consecutive": 0, "limit": None}))
    on = optim.AdamW(lin.parameters(), skip_grad_norm=3.0)
    assert on.guard_on is True and on.skip_grad_norm == 3.0
    sd = on.state_dict()
    assert sd["guard"] == {"skipped": 0, "consecutive": 0, "limit": 3.0}
    on.load_state_dict(dict(sd, guard={"skipped": 4, "consecutive": 2, "limit": None}))
    assert on.skipped_steps() == 4 and on.consecutive_skips() == 2 and on.skip_grad_norm is None
    assert on.state_dict()["guard"] == {"skipped": 4, "consecutive": 2, "limit": None}
    on.load_state_dict({k: v for k, v in sd.items() if k != "guard"})          # the guard turned on mid-run: counters start at 0
    assert on.skipped_steps() == 0 and on.consecutive_skips() == 0
    for bad in ({"skipped": 1, "consecutive": 0}, {"skipped": -1, "consecutive": 0, "limit": None},
                {"skipped": 1, "consecutive": True, "limit": None}, {"skipped": 1, "consecutive": 0, "limit": 0.0}):
        with pytest.raises(ValueError, match="guard|skip_grad_norm"):
            on.load_state_dict(dict(sd, guard=bad))


def test_meta_rules_in_the_three_directions():
    from drakegpt_amd import checkpoint as CK
    # unguarded file: into an unguarded and into a guarded engine
    for meta in ({}, {"precision": "bf16"}, {"update_guard": False}):
        CK.check_guard_meta(meta, False)
        CK.check_guard_meta(meta, True)
    # guarded file: into a guarded engine; refused, naming the field, by an engine without the guard
    CK.check_guard_meta({"update_guard": True}, True)
    with pytest.raises(ValueError, match=r"meta\.update_guard differs"):
        CK.check_guard_meta({"update_guard": True}, False)
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match=r"meta\.update_guard"):
            CK.check_guard_meta({"update_guard": bad}, True)


def test_engine_section_rules():
    from drakegpt_amd import checkpoint as CK
    good = {"skipped": 3, "consecutive": 1, "limit": 2.0, "opt_step": 7}
    on, off = {"update_guard": True}, {}
    assert CK.check_guard_state(None, off, False, 10) is None
    assert CK.check_guard_state(None, off, True, 10) == (None, 0, 0, None, False)          # opt_step := step_word, counters 0
    assert CK.check_guard_state(good, on, True, 10) == (7, 3, 1, 2.0, True)
    assert CK.check_guard_state(dict(good, limit=None), on, True, 10) == (7, 3, 1, None, True)
    with pytest.raises(ValueError, match=r"meta\.update_guard differs"):
        CK.check_guard_state(good, on, False, 10)
    for section, meta, what in ((good, off, r"engine\.guard"), (None, on, r"engine\.guard"), ([1], on, r"engine\.guard"),
                                ({k: v for k, v in good.items() if k != "opt_step"}, on, r"engine\.guard\.opt_step"),
                                (dict(good, skipped=-1), on, r"engine\.guard\.skipped"), (dict(good, skipped=True), on, r"engine\.guard\.skipped"),
                                (dict(good, consecutive=4), on, r"engine\.guard\.consecutive"), (dict(good, opt_step=11), on, r"engine\.guard\.opt_step"),
                                (dict(good, opt_step=1.0), on, r"engine\.guard\.opt_step"), (dict(good, limit=0.0), on, r"engine\.guard\.limit"),
                                (dict(good, limit=float("nan")), on, r"engine\.guard\.limit")):
        with pytest.raises(ValueError, match=what):
            CK.check_guard_state(section, meta, True, 10)


def _stub(**kw):
    base = dict(model=types.SimpleNamespace(precision="fp32", context_length=8), V=80, C=32, L=3, NH=4, B=16, T=8, accum=1, world=1,
                p_drop=0.0, _loss_kw={}, ignore_index=None, ema=None, guard=None)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_default_engine_meta_has_no_new_key():
    from drakegpt_amd.engine import TrainEngine
    plain = TrainEngine._meta(_stub())
    assert sorted(plain) == sorted(["precision", "vocab_size", "embedding_dim", "num_layers", "num_heads", "model_context_length",
                                    "batch_size", "context_length", "accum_steps", "world_size", "dropout"])
    guarded = TrainEngine._meta(_stub(guard=object()))
    assert guarded == dict(plain, update_guard=True)
    assert "guard" not in TrainEngine._ENGINE_KEYS          # a file without the section stays loadable


def test_train_flags(capsys):
    from drakegpt_amd import train
    a = train.parse_args(["--model", "BlocksLM"])
    assert a.skip_nonfinite is False and a.skip_grad_norm is None and a.max_consecutive_skips == 25
    plain = train.run_args(a, 1, 1)
    assert not any("skip" in k or "guard" in k for k in plain)          # a run without the flags writes what it wrote before
    a = train.parse_args(["--model", "BlocksLM", "--skip-nonfinite"])
    assert a.skip_nonfinite is True and a.skip_grad_norm is None
    a = train.parse_args(["--model", "BlocksLM", "--skip-grad-norm", "1e-9", "--max-consecutive-skips", "3"])
    assert a.skip_nonfinite is True and a.skip_grad_norm == 1e-9 and a.max_consecutive_skips == 3
    assert train.run_args(a, 1, 1) == plain          # the guard may be turned on for a resumed run
    for bad in (["--skip-grad-norm", "0"], ["--skip-grad-norm", "nan"], ["--skip-grad-norm", "inf"], ["--skip-grad-norm", "-1"],
                ["--skip-grad-norm", "lots"], ["--max-consecutive-skips", "-1"]):
        with pytest.raises(SystemExit) as ei:
            train.parse_args(["--model", "BlocksLM"] + bad)
        assert ei.value.code == 2
        assert "--skip-grad-norm" in capsys.readouterr().err or bad[0] == "--max-consecutive-skips"
