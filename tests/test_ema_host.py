"""CPU: the restatement of the weights' moving average (tests/ema_model.py) against its fp64 form and against torch's
AveragedModel, the warm-up schedule, and every check of the feature that runs without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_model as EM  # noqa: E402


def _sequence(k, n, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n, generator=g)
    return [(base + 0.05 * (i + 1) * torch.randn(n, generator=g)).numpy() for i in range(k)]


@pytest.mark.parametrize("decay,warmup", [(0.99, False), (0.9, False), (0.999, True)])
def test_fp32_model_against_fp64_and_averaged_model(decay, warmup):
    """after k steps the fp32 recurrence is within 2 k 2^-24 max|p| of the fp64 one: every step adds one half-ulp rounding of a
    value <= max|p| in the final add (2^-24 max|p|) and two much smaller ones (the difference and the product, scaled by w).
    torch's CPU lerp contracts to an FMA, so AveragedModel differs in the last bit: the same bound, not equality."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    k, n = 20, 4099
    ps = _sequence(k, n, seed=3)
    bound = 2 * k * 2.0 ** -24 * max(float(np.abs(p).max()) for p in ps)
    e32 = EM.run(ps, decay, warmup)
    e64 = EM.run(ps, decay, warmup, fn=EM.step64)
    assert e32.dtype == np.float32 and e64.dtype == np.float64
    err = float(np.abs(e32.astype(np.float64) - e64).max())
    print(f"decay {decay} warmup {warmup}: fp32 vs fp64 {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float(np.abs(e32 - ps[-1]).max()) > 100 * bound          # (the average is not simply the last weights)
    if not warmup:                                                  # torch's helper has no warm-up
        lin = torch.nn.Linear(n, 1, bias=False)
        avg = AveragedModel(lin, multi_avg_fn=get_ema_multi_avg_fn(decay))
        for p in ps:
            with torch.no_grad():
                lin.weight.copy_(torch.from_numpy(p).view(1, n))
            avg.update_parameters(lin)
        t = avg.module.weight.detach().view(n).numpy()
        err_t = float(np.abs(e32.astype(np.float64) - t.astype(np.float64)).max())
        print(f"decay {decay}: fp32 model vs AveragedModel {err_t:.3e}")
        assert err_t <= bound
        assert float(np.abs(t.astype(np.float64) - e64).max()) <= bound


def test_first_step_does_not_read_the_buffer():
    p = np.arange(5, dtype=np.float32)
    assert np.array_equal(EM.step(np.full(5, np.nan, dtype=np.float32), p, 0.9, False, 0), p)
    assert np.array_equal(EM.step(None, p, 0.9, True, 0), p)


def test_warmup_schedule():
    want = {0: 0.1, 5: 0.4, 80: 0.9, 81: 0.9, 1000: 0.9, 2 ** 24: 0.9}
    for s, d in want.items():
        got = EM.decay_at(0.9, True, s)
        assert got.dtype == np.float32 and got == np.float32(d), (s, got)
    assert EM.decay_at(0.9, True, 0) == np.float32(1) / np.float32(10)
    assert EM.decay_at(0.9, True, 5) == np.float32(6) / np.float32(15)
    assert EM.decay_at(0.9, True, 80) == np.float32(0.9) and np.float32(81) / np.float32(90) == np.float32(0.9)
    assert EM.decay_at(0.9, True, 79) < np.float32(0.9)
    assert all(EM.decay_at(0.9, False, s) == np.float32(0.9) for s in (0, 5, 80))
    assert EM.weight(0.9, True, 5) == np.float32(1) - np.float32(6) / np.float32(15)


def test_check_ema_options():
    from drakegpt_amd import ops
    assert ops.check_ema_options() is None and ops.check_ema_options(None, False) is None
    assert ops.check_ema_options(0.99) == 0.99 and ops.check_ema_options(0.5, True) == 0.5
    assert isinstance(ops.check_ema_options(np.float32(0.5)), float)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf"), True, False, "x", [0.9], 1.0 - 1e-12):
        with pytest.raises(ValueError, match="ema_decay"):
            ops.check_ema_options(bad)
    with pytest.raises(ValueError, match="ema_warmup goes with ema_decay"):
        ops.check_ema_options(None, True)
    with pytest.raises(ValueError, match="ema_decay"):
        ops.new_ema_hyper(None, False, "cpu")
    assert ops.new_ema_hyper(0.75, True, "cpu").tolist() == [0.75, 1.0] and ops.new_ema_hyper(0.75, False, "cpu").tolist() == [0.75, 0.0]


def test_layers_check_before_touching_a_device():
    import drakegpt_amd as D
    from drakegpt_amd import optim
    lin = torch.nn.Linear(3, 3)
    for kw in (dict(ema_decay=1.0), dict(ema_decay=True), dict(ema_warmup=True), dict(ema_decay=float("nan"))):
        with pytest.raises(ValueError, match="ema_"):
            optim.AdamW(lin.parameters(), **kw)
    opt = optim.AdamW(lin.parameters())
    assert opt.ema_decay is None and "ema" not in opt.state_dict()
    with pytest.raises(RuntimeError, match="without a moving average"):
        with opt.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="without a moving average"):
        opt.set_ema_decay(0.9)
    with pytest.raises(ValueError, match="ema differs"):
        opt.load_state_dict(dict(opt.state_dict(), ema={"decay": 0.9, "warmup": False, "values": {}}))
    on = optim.AdamW(lin.parameters(), ema_decay=0.9)
    sd = on.state_dict()
    assert sd["ema"] == {"decay": 0.9, "warmup": False, "values": {}}
    on.load_state_dict(sd)
    with pytest.raises(ValueError, match="ema differs"):
        on.load_state_dict({k: v for k, v in sd.items() if k != "ema"})
    assert D.optim.AdamW is optim.AdamW


def test_train_flags(capsys):
    from drakegpt_amd import train
    a = train.parse_args(["--model", "BlocksLM"])
    assert a.ema_decay is None and a.ema_warmup is False
    mm = train.run_args(a, 1, 1)
    assert mm["ema_decay"] is None and mm["ema_warmup"] is False
    assert train.RUN_ARG_DEFAULTS["ema_decay"] is None and train.RUN_ARG_DEFAULTS["ema_warmup"] is False
    a = train.parse_args(["--model", "BlocksLM", "--ema-decay", "0.99", "--ema-warmup"])
    mm = train.run_args(a, 1, 1)
    assert (a.ema_decay, a.ema_warmup) == (0.99, True) and mm["ema_decay"] == 0.99 and mm["ema_warmup"] is True
    for bad in (["--ema-decay", "1.0"], ["--ema-decay", "0"], ["--ema-decay", "nan"], ["--ema-decay", "lots"], ["--ema-warmup"]):
        with pytest.raises(SystemExit) as ei:
            train.parse_args(["--model", "BlocksLM"] + bad)
        assert ei.value.code == 2
        assert "--ema-" in capsys.readouterr().err


def test_resume_must_repeat_the_ema_options(tmp_path):
    from drakegpt_amd import checkpoint as CK
    from drakegpt_amd import train
    path = str(tmp_path / "s.pt")
    base = ["--model", "BlocksLM", "--precision", "fp32"]
    plain = train.run_args(train.parse_args(base), 1, 1)
    opt = train.run_args(train.parse_args(base + ["--ema-decay", "0.9"]), 1, 1)

    def write(mm):
        CK.save_train_state(path, {"format": CK.FORMAT, "version": CK.VERSION, "iteration": 4, "sched_steps": 1,
                                   "rng_state": torch.get_rng_state(), "args": mm, "engine": None, "model": {}, "optimizer": {}})
    write({k: v for k, v in plain.items() if k not in ("ema_decay", "ema_warmup")})          # a file written before the flags existed
    assert train.load_run_state(path, plain)["iteration"] == 4
    with pytest.raises(SystemExit, match="ema_decay differs.*None.*0.9"):
        train.load_run_state(path, opt)
    with pytest.raises(SystemExit, match="ema_warmup"):
        train.load_run_state(path, dict(plain, ema_warmup=True))
    write(opt)
    assert train.load_run_state(path, opt)["iteration"] == 4
    with pytest.raises(SystemExit, match="ema_decay"):
        train.load_run_state(path, plain)
    with pytest.raises(SystemExit, match="ema_decay"):
        train.load_run_state(path, dict(opt, ema_decay=0.99))


def test_meta_refusals():
    """whether an average is kept must agree in both directions; a file written before the field existed reads as off"""
    from drakegpt_amd import checkpoint as CK
    CK.check_ema_meta({}, False)
    CK.check_ema_meta({"precision": "bf16"}, False)
    CK.check_ema_meta({"ema": True}, True)
    CK.check_ema_meta({"ema": False}, False)
    for saved, own in (({}, True), ({"ema": True}, False), ({"ema": False}, True), ({"ema": 1}, True), ({"ema": "yes"}, True)):
        with pytest.raises(ValueError, match=r"meta\.ema differs"):
            CK.check_ema_meta(saved, own)
    # the engine section
    vals = torch.zeros(7)
    good = {"decay": 0.9, "warmup": True, "values": vals}
    assert CK.check_ema_state(None, False, 7) is None
    d, w, v = CK.check_ema_state(good, True, 7)
    assert (d, w) == (0.9, True) and v is vals
    for section, own, what in ((good, False, r"engine\.ema differs"), (None, True, r"engine\.ema differs"),
                               ({"decay": 0.9, "warmup": True}, True, r"engine\.ema\.values"),
                               (dict(good, decay=1.0), True, r"engine\.ema\.decay"), (dict(good, decay=None), True, r"engine\.ema\.decay"),
                               (dict(good, warmup=1), True, r"engine\.ema\.warmup"), (dict(good, values=vals[:6]), True, r"engine\.ema\.values"),
                               (dict(good, values=vals.double()), True, r"engine\.ema\.values"), ([1], True, r"engine\.ema")):
        with pytest.raises(ValueError, match=what):
            CK.check_ema_state(section, own, 7)
