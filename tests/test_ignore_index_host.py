"""CPU: the fp64 statement of ignore_index (tests/ignore_model.py) against torch's own F.cross_entropy(ignore_index=), the numpy
restatement of the count launch, and the plain-Python checks (check_loss_options, check_ids(allow=), the train parser)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ignore_model as IM  # noqa: E402
import loss_model as LM  # noqa: E402

OPTS = [(0.0, 0.0), (0.125, 0.0), (0.125, 1e-2)]


@pytest.mark.parametrize("M,V", [(48, 80), (33, 7), (1000, 80)])
def test_formula_is_torchs_cross_entropy(M, V):
    """loss and gradient, every pattern, I = -100 and I = 3, to 1e-12 in fp64 (eps = 0.125 is exact in the single precision torch
    carries label_smoothing in); the z-loss term restated with torch over the rows that count"""
    x, t0 = LM.edge_case_logits(M, V, seed=M + V)
    cases = IM.cases(M, V)
    assert {p for p, _, _ in cases} == set(IM.PATTERNS)
    for pattern, I, ig in cases:
        t = IM.apply_mask(t0, ig, I, V)
        assert torch.equal(t == I, ig)
        for eps, zeta in OPTS:
            xd = x.double().requires_grad_(True)
            keep = t != I
            want = torch.nn.functional.cross_entropy(xd, t, ignore_index=I, label_smoothing=eps)
            if zeta:
                want = want + zeta * (torch.logsumexp(xd, 1).pow(2) * keep).sum() / keep.sum()
            (3.0 * want).backward()
            rows, loss, g, k = IM.masked_objective_fp64(x, t, I, eps, zeta, grad_scale=3.0)
            assert torch.equal(k, keep)
            assert abs(loss.item() - want.item()) < 1e-12, (pattern, I, eps, zeta)
            assert (g - xd.grad).abs().max().item() < 1e-12, (pattern, I, eps, zeta)
            assert torch.all(rows[ig] == 0) and torch.all(g[ig] == 0)


def test_all_rows_ignored_is_nan_with_zero_gradient():
    x, t = LM.edge_case_logits(8, 80, seed=1)
    t[:] = -100
    rows, loss, g, keep = IM.masked_objective_fp64(x, t, -100, 0.125, 1e-2)
    assert torch.isnan(loss) and not keep.any() and torch.all(g == 0) and torch.all(rows == 0)
    assert torch.isnan(torch.nn.functional.cross_entropy(x.double(), t, ignore_index=-100))


def test_count_restatement():
    for n in (0, 1, 3, 33, 1000, 16384, 16383):
        c = IM.count_np(n)
        assert c.dtype == np.float32 and c[0] == n
        if n == 0:
            assert np.isinf(c[1]) and c[1] > 0
        else:
            # one correctly rounded division: the fp32 nearest to the fp64 quotient (exact to 2^-53, far inside half an fp32 ulp)
            assert c[1] == np.float32(1.0 / n)
    assert IM.count_np(3)[1].tobytes() == np.float32(0.33333334).tobytes()


def test_check_loss_options_ignore_index():
    from drakegpt_amd.ops import check_loss_options
    assert check_loss_options(0.125, 1e-2) == (0.125, 1e-2)                       # the two-option form: what it always returned
    assert check_loss_options(0.125, 1e-2, None) == (0.125, 1e-2, None)
    assert check_loss_options(ignore_index=-100) == (0.0, 0.0, -100)
    assert check_loss_options(ignore_index=np.int64(3))[2] == 3 and type(check_loss_options(ignore_index=np.int64(3))[2]) is int
    for I in (-(1 << 63), (1 << 63) - 1, 0):
        assert check_loss_options(ignore_index=I)[2] == I
    for bad in (True, False, 3.0, -100.0, "3", 1 << 63, -(1 << 63) - 1, [3]):
        with pytest.raises(ValueError, match="ignore_index"):
            check_loss_options(ignore_index=bad)
    with pytest.raises(ValueError, match="label_smoothing"):
        check_loss_options(1.0, 0.0, -100)


def test_check_ids_allow():
    from drakegpt_amd.ops import check_ids
    t = torch.tensor([0, 5, -100, 79, -100])
    with pytest.raises(IndexError):
        check_ids(t, 80, "targets")
    check_ids(t, 80, "targets", allow=-100)
    check_ids(torch.tensor([-100, -100]), 80, "targets", allow=-100)                # nothing but ignored targets
    check_ids(torch.tensor([0, 3, 79]), 80, "targets", allow=3)                    # an in-vocabulary value: an ordinary token
    with pytest.raises(IndexError, match=r"\[-1, 79\]"):
        check_ids(torch.tensor([0, -1, -100, 79]), 80, "targets", allow=-100)      # -1 stays an error, as in torch
    with pytest.raises(IndexError):
        check_ids(torch.tensor([0, 80, -100]), 80, "targets", allow=-100)
    with pytest.raises(IndexError):
        check_ids(torch.tensor([0, -100]), 80, "targets", allow=3)


def test_models_take_the_option_without_a_device():
    import drakegpt_amd as D
    m = D.BigramLM(80)
    assert m.ignore_index is None
    assert m.set_loss_options(ignore_index=-100) is m and m.ignore_index == -100 and m.label_smoothing == 0.0
    m.set_loss_options(0.125)
    assert m.ignore_index is None                                                 # every call states all three
    with pytest.raises(ValueError, match="ignore_index"):
        m.set_loss_options(ignore_index=1.5)


def test_train_parser_takes_ignore_token():
    from drakegpt_amd import train
    base = ["--model", "TransformerLM", "--iters", "4"]
    a = train.parse_args(base)
    assert a.ignore_token is None and "ignore_token" not in train.run_args(a, 1, 1)      # the must-match set a run always wrote
    a = train.parse_args(base + ["--ignore-token", "3"])
    assert a.ignore_token == 3 and train.run_args(a, 1, 1)["ignore_token"] == 3
    assert train.parse_args(base + ["--ignore-token", "-100"]).ignore_token == -100
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--ignore-token", "1.5"])
