"""CPU: the sampler's numpy restatement (tests/sampling_model.py) checks itself statistically, and generate()'s new keyword
arguments are validated in plain Python before anything touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampling_model as SM  # noqa: E402

# seed, L, V, top_k, temperature, logit scale, rows -- rows of IDENTICAL logits (randn, seed 3)
CASES = [
    (1234, 5, 80, None, 1.0, 1.0, 8192),
    (1234, 6, 80, 10, 0.7, 1.0, 8192),
    (7, 300, 80, None, 1.0, 1.0, 8192),
    (1234, 5, 50257, 50, 1.0, 1.0, 4096),
    (1234, 5, 50257, None, 1.0, 8.0, 4096),
]


def case_logits(V, scale):
    g = torch.Generator().manual_seed(3)
    return (torch.randn(V, generator=g) * scale).numpy().astype(np.float32)


@pytest.mark.parametrize("seed,L,V,top_k,temperature,scale,rows", CASES)
def test_restatement_frequencies_follow_its_distribution(seed, L, V, top_k, temperature, scale, rows):
    """N draws of a token with probability p land within 5 binomial standard deviations of p (+ 1/N for the discreteness of
    a frequency) -- a bound from the binomial law, 80 .. 50257 tokens at once: P(any failure) < 50257 * 6e-7."""
    x = case_logits(V, scale)
    p, kept = SM.probs(x, temperature, top_k)
    toks = SM.sample(x, seed, L, temperature, top_k, rows=rows)
    assert toks.shape == (rows,) and kept[toks].all()
    if top_k is not None:
        assert kept.sum() == top_k                      # randn: no ties at the threshold
    ok, worst = SM.freq_bound_ok(toks, p)
    print(f"worst standardised deviation {worst:.2f} sigma")
    assert ok, worst


def test_uniforms_are_uniform():
    """row 0 over L = 0 .. 4095: Kolmogorov-Smirnov distance below 1.95 / sqrt(N) = 0.030 (the 0.1 % critical value)"""
    u = np.sort(np.array([SM.uniforms(1234, L, 1)[0] for L in range(4096)]))
    n = u.size
    D = max(np.max(np.arange(1, n + 1) / n - u), np.max(u - np.arange(n) / n))
    print(f"KS distance {D:.4f}")
    assert 0.0 <= u[0] and u[-1] < 1.0
    assert D < 1.95 / np.sqrt(n)


def test_restatement_edge_semantics():
    x = np.array([0.5, 2.0, -np.inf, 2.0, 1.0, 1.0, -3.0], dtype=np.float32)
    assert SM.sample(x, 1, 0, temperature=0, rows=3).tolist() == [1, 1, 1]            # greedy: lowest index among the maxima
    p, kept = SM.probs(x, 1.0, 3)                                                     # 3rd largest is 1.0, twice: both kept
    assert kept.tolist() == [False, True, False, True, True, True, False]
    assert abs(p.sum() - 1) < 1e-15 and p[2] == 0
    toks = SM.sample(x, 5, 9, rows=4096)
    assert 2 not in toks                                                              # -inf is never sampled
    p1, kept1 = SM.probs(x, 1.0, 1)                                                   # top_k = 1 with tied maxima keeps both
    assert kept1.sum() == 2
    pV, keptV = SM.probs(x, 1.0, x.size)
    p0, kept0 = SM.probs(x, 1.0, None)
    assert (pV == p0).all() and (keptV == kept0).all()                                # top_k = V is "off"


def _lm():
    import drakegpt_amd as D
    return D.TransformerLM(80, 32, 8, 4, 1, 0.0).eval()


@pytest.mark.parametrize("kw", [dict(sampler="gpu"), dict(sampler=None), dict(temperature=-0.5), dict(temperature=float("nan")),
                                dict(temperature=float("inf")), dict(top_k=0), dict(top_k=-3), dict(top_k=2.5)])
@pytest.mark.parametrize("cls", ["TransformerLM", "BigramLM"])
def test_generate_rejects_bad_sampling_arguments_before_the_device(cls, kw):
    import drakegpt_amd as D
    m = _lm() if cls == "TransformerLM" else D.BigramLM(80)
    idx = torch.zeros((1, 1), dtype=torch.long)              # a CPU tensor: a valid call would fail with "must be on the GPU"
    with pytest.raises(ValueError):
        m.generate(idx, 2, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(sampler="device"), dict(temperature=0.0), dict(top_k=10 ** 6, temperature=0.5)])
def test_valid_sampling_arguments_reach_the_gpu_check(kw):
    """valid arguments (a top_k above V is clamped, temperature 0 is greedy) get as far as the "needs a GPU" error"""
    with pytest.raises(RuntimeError, match="GPU"):
        _lm().generate(torch.zeros((1, 1), dtype=torch.long), 2, **kw)


def test_check_sampling_args_clamps_top_k():
    from drakegpt_amd.model import check_sampling_args
    assert check_sampling_args("host", 1, None, 80) == (1.0, None)
    assert check_sampling_args("device", 0, 500, 80) == (0.0, 80)
    assert check_sampling_args("device", 0.7, 5, 80) == (0.7, 5)


def test_train_parser_has_the_sampling_flags():
    from drakegpt_amd import train
    a = train.build_parser().parse_args([])
    assert (a.sampler, a.temperature, a.top_k) == ("host", 1.0, None)
    a = train.build_parser().parse_args(["--sampler", "device", "--temperature", "0.8", "--top-k", "40"])
    assert (a.sampler, a.temperature, a.top_k) == ("device", 0.8, 40)
