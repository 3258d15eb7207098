"""CPU: the fp64 restatement of the loss options (tests/loss_model.py) against torch, the argument checks of every layer that
can run without a GPU, and the bound |g| <= grad_scale on which the fp8 gradient copy's a-priori scale rests."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_model as LM  # noqa: E402

SHAPES = [(33, 7), (48, 80), (20, 300), (8, 4099)]


@pytest.mark.parametrize("M,V", SHAPES)
@pytest.mark.parametrize("zeta", [0.0, 1e-2])
def test_restatement_equals_torch_in_fp64(M, V, zeta):
    """eps = 0.125 is exact in fp32, the precision torch carries label_smoothing in: loss to 1e-14, gradient to 1e-14"""
    x, t = LM.edge_case_logits(M, V, seed=V)
    xd = x.double().requires_grad_(True)
    loss = LM.objective_torch(xd, t, 0.125, zeta)
    loss.backward()
    rows, g = LM.objective_fp64(x, t, 0.125, zeta, grad_scale=1.0 / M)
    assert abs(rows.mean().item() - loss.item()) < 1e-13 * max(1.0, abs(loss.item()))
    assert (g - xd.grad).abs().max().item() < 1e-14
    # ... and with both options off it is the plain cross entropy
    rows0, g0 = LM.objective_fp64(x, t, grad_scale=1.0 / M)
    xd.grad = None
    plain = torch.nn.functional.cross_entropy(xd, t)
    plain.backward()
    assert abs(rows0.mean().item() - plain.item()) < 1e-13 * max(1.0, plain.item()) and (g0 - xd.grad).abs().max().item() < 1e-14


def test_gradient_rows_sum_to_the_z_term():
    """a row sums to 2 zeta lse grad_scale: zero without z-loss, smoothing or not"""
    x, t = LM.edge_case_logits(20, 300, seed=1)
    lse = torch.logsumexp(x.double(), 1)
    for eps, zeta in ((0.0, 0.0), (0.125, 0.0), (0.0, 1e-2), (0.125, 1e-2)):
        _, g = LM.objective_fp64(x, t, eps, zeta, grad_scale=0.25)
        assert (g.sum(1) - 2 * zeta * lse * 0.25).abs().max().item() < 1e-14


def test_check_loss_options():
    from drakegpt_amd import ops
    assert ops.check_loss_options() == (0.0, 0.0)
    assert ops.check_loss_options(0.125, 1e-2) == (0.125, 1e-2)
    assert ops.check_loss_options(0, 3) == (0.0, 3.0)
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="label_smoothing"):
            ops.check_loss_options(bad, 0.0)
    for bad in (-1e-3, float("nan"), float("inf"), "x", None, False):
        with pytest.raises(ValueError, match="z_loss"):
            ops.check_loss_options(0.0, bad)


def test_layers_check_before_touching_a_device():
    """the checks are plain Python at every layer: raised on CPU tensors, before the GPU-only checks"""
    import drakegpt_amd as D
    from drakegpt_amd import functional as HF
    from drakegpt_amd import ops
    x, t = torch.zeros(4, 7), torch.zeros(4, dtype=torch.long)
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.cross_entropy(x, t, 7, label_smoothing=1.0)
    with pytest.raises(ValueError, match="z_loss"):
        ops.cross_entropy(x, t, 7, z_loss=-1.0)
    with pytest.raises(ValueError, match="label_smoothing"):
        ops.cross_entropy_fp8(x, t, 7, x, 1.0, x, label_smoothing=-0.5)
    with pytest.raises(TypeError):
        ops.cross_entropy_fp8(x, t, 7, x, 1.0, x, z_loss=0.01)              # the fp8 entry has no z argument
    with pytest.raises(ValueError, match="z_loss"):
        ops.cross_entropy_fused(x, t, 7, x, 1.0, None, 0, 2, None, None, 1.0, z_loss=float("inf"))
    with pytest.raises(ValueError, match="label_smoothing"):
        HF.cross_entropy(x, t, 2.0, 0.0)
    for m in (D.BigramLM(7), D.TransformerLM(7, 8, 4, 2, 1, 0.0)):
        assert (m.label_smoothing, m.z_loss) == (0.0, 0.0)
        with pytest.raises(ValueError, match="z_loss"):
            m.set_loss_options(0.1, -2.0)
        assert (m.label_smoothing, m.z_loss) == (0.0, 0.0)
        assert m.set_loss_options(0.125, 1e-2) is m and (m.label_smoothing, m.z_loss) == (0.125, 1e-2)
        assert not any("smooth" in k or "z_loss" in k for k in m.state_dict())          # plain attributes
        m.set_loss_options()
        assert (m.label_smoothing, m.z_loss) == (0.0, 0.0)


def test_train_flags(capsys):
    from drakegpt_amd import train
    a = train.parse_args(["--model", "BlocksLM"])
    assert (a.label_smoothing, a.z_loss) == (0.0, 0.0)
    a = train.parse_args(["--model", "BlocksLM", "--label-smoothing", "0.125", "--z-loss", "1e-2"])
    assert (a.label_smoothing, a.z_loss) == (0.125, 1e-2)
    mm = train.run_args(a, 1, 1)
    assert mm["label_smoothing"] == 0.125 and mm["z_loss"] == 1e-2
    assert train.RUN_ARG_DEFAULTS["label_smoothing"] == 0.0 and train.RUN_ARG_DEFAULTS["z_loss"] == 0.0
    for bad in (["--label-smoothing", "1.0"], ["--label-smoothing", "-0.1"], ["--z-loss", "-1"], ["--z-loss", "nan"],
                ["--label-smoothing", "lots"]):
        with pytest.raises(SystemExit) as ei:
            train.parse_args(["--model", "BlocksLM"] + bad)
        assert ei.value.code == 2
        assert bad[0] in capsys.readouterr().err


def test_resume_must_repeat_the_loss_options(tmp_path):
    from drakegpt_amd import checkpoint as CK
    from drakegpt_amd import train
    path = str(tmp_path / "s.pt")
    base = ["--model", "BlocksLM", "--precision", "fp32"]
    plain = train.run_args(train.parse_args(base), 1, 1)
    opt = train.run_args(train.parse_args(base + ["--label-smoothing", "0.125", "--z-loss", "1e-2"]), 1, 1)

    def write(mm):
        CK.save_train_state(path, {"format": CK.FORMAT, "version": CK.VERSION, "iteration": 4, "sched_steps": 1,
                                   "rng_state": torch.get_rng_state(), "args": mm, "engine": None, "model": {}, "optimizer": {}})
    write({k: v for k, v in plain.items() if k not in ("label_smoothing", "z_loss")})          # a file written before the flags existed
    assert train.load_run_state(path, plain)["iteration"] == 4
    for field in ("label_smoothing", "z_loss"):
        with pytest.raises(SystemExit, match=field):
            train.load_run_state(path, dict(plain, **{field: opt[field]}))
    write(opt)
    assert train.load_run_state(path, opt)["iteration"] == 4
    with pytest.raises(SystemExit, match="label_smoothing"):
        train.load_run_state(path, plain)


def _near_one_hot(M, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, V, generator=g)
    hot = torch.randint(0, V, (M,), generator=g)
    x[torch.arange(M), hot] += 40.0
    t = hot.clone()
    t[::2] = torch.randint(0, V, (M,), generator=g)[::2]          # half of the targets on the peak, half anywhere
    return x, t


def test_smoothing_keeps_the_fp8_bound_and_z_loss_breaks_it():
    """the e5m2 copy of the gradient is scaled a priori by 57344 / grad_scale: that needs |g_i| <= grad_scale.  Smoothing alone keeps
    it (|p_i - eps / V| < 1, |p_t - (1 - eps) - eps / V| < 1); zeta = 0.01 does not -- why dg_cross_entropy_fp8_smooth has no z"""
    gs = 0.25
    worst_z = 0.0
    for V in (7, 80, 4099):
        for x, t in (LM.edge_case_logits(64, V, seed=V), LM.edge_case_logits(64, V, seed=V + 1, scale=8.0), _near_one_hot(64, V, V)):
            for eps in (0.0, 0.125, 0.5, 0.99):
                _, g = LM.objective_fp64(x, t, eps, 0.0, grad_scale=gs)
                assert g.abs().max().item() <= gs
            _, g = LM.objective_fp64(x, t, 0.125, 1e-2, grad_scale=gs)
            worst_z = max(worst_z, g.abs().max().item() / gs)
    assert worst_z > 1.0, worst_z
