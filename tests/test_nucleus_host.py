"""CPU: the top-p / min-p restatement (tests/nucleus_model.py) against an independent brute force and hand-made rows; the new
arguments of generate() are validated in plain Python before anything touches a device; the parameter block's packing."""
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nucleus_model as NM  # noqa: E402
import sampling_model as SM  # noqa: E402


def brute_kept(logits_row, temperature, top_k, top_p, min_p):
    """the rule read off a descending stable sort: exclusive cumulative mass in Python ints, tie groups sharing one G"""
    x = np.asarray(logits_row, dtype=np.float32)
    z = (x * SM.inv_temp(temperature)).astype(np.float32)
    V = z.size
    order = sorted(range(V), key=lambda j: -float(z[j]))          # sorted() is stable
    k0 = [False] * V
    if top_k is not None and 0 < top_k < V:
        tau = z[order[top_k - 1]]
        for j in range(V):
            k0[j] = bool(z[j] >= tau) and z[j] > -np.inf
    else:
        k0 = [bool(z[j] > -np.inf) for j in range(V)]
    mx = z.max()
    e = [float(np.exp(np.float64(np.float32(z[j] - mx)))) if k0[j] else 0.0 for j in range(V)]
    mp = float(np.float32(min_p)) if min_p is not None else 0.0
    k1 = [k0[j] and (mp == 0.0 or e[j] >= mp) for j in range(V)]
    if top_p is None or float(np.float32(top_p)) >= 1.0:
        return np.array(k1)
    w = [int(np.rint(e[j] * 2.0 ** 40)) if k1[j] else 0 for j in range(V)]
    S1 = sum(w)
    T = float(np.float32(top_p)) * float(S1)
    kept = [False] * V
    run, i = 0, 0                                                  # run = mass of everything strictly above the current tie group
    while i < V:
        g = i
        while g < V and z[order[g]] == z[order[i]]:
            g += 1
        for j in order[i:g]:
            kept[j] = k1[j] and float(run) < T
        run += sum(w[j] for j in order[i:g])
        i = g
    return np.array(kept)


@pytest.mark.parametrize("seed,V,temperature,top_k,top_p,min_p", [
    (1, 80, 1.0, None, 0.9, None),
    (2, 80, 0.7, 10, 0.5, None),
    (3, 300, 1.3, None, 0.3, 0.01),
    (4, 300, 1.0, 40, 0.95, 0.2),
    (5, 1000, 1.0, None, 0.999, None),
    (6, 80, 1.0, None, None, 0.1),
    (7, 80, 1.0, 5, 1e-6, None),
])
def test_restatement_equals_the_brute_force(seed, V, temperature, top_k, top_p, min_p):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((6, V)) * 3).astype(np.float32)
    x[1] = np.round(x[1])                      # many ties
    x[2, ::3] = -np.inf
    x[3] = np.round(x[3] * 2) / 2
    x[3, 5::7] = -np.inf
    e, kept = NM.weights(x, temperature, top_k, top_p, min_p)
    for m in range(x.shape[0]):
        want = brute_kept(x[m], temperature, top_k, top_p, min_p)
        assert (kept[m] == want).all(), m
        assert kept[m, np.argmax(x[m])]
    e0, k0 = SM.weights(x, temperature, top_k)
    assert (e == np.where(kept, e0, 0.0)).all() and not (kept & ~k0).any()


@pytest.mark.parametrize("name", list(NM.hand_rows()))
def test_hand_made_rows(name):
    x, kw, want = NM.hand_rows()[name]
    e, kept = NM.weights(x, **kw)
    if want is None:
        assert kept.all()
    elif want == "finite":
        assert kept.any() and not kept[~np.isfinite(x)].any()
        assert kept.sum() < np.isfinite(x).sum()                  # and the filter did something
        toks = NM.sample(x, 3, 9, rows=2048, **kw)
        assert kept[toks].all()
    else:
        assert np.flatnonzero(kept).tolist() == want
    assert (kept == brute_kept(x, kw.get("temperature", 1.0), kw.get("top_k"), kw.get("top_p"), kw.get("min_p"))).all()


def test_min_p_one_keeps_the_maxima():
    x = np.array([0.5, 2.0, -np.inf, 2.0, 1.0], dtype=np.float32)
    for kw in (dict(min_p=1.0), dict(min_p=1.0, top_p=0.999)):
        assert NM.weights(x, **kw)[1].tolist() == [False, True, False, True, False]          # exp(0) = 1 >= 1, exactly


def test_off_is_sampling_model():
    x = (np.random.default_rng(8).standard_normal((5, 257)) * 3).astype(np.float32)
    x[2, 7] = -np.inf
    for top_k in (None, 10):
        e0, k0 = SM.weights(x, 0.7, top_k)
        for kw in (dict(), dict(top_p=1.0), dict(min_p=0.0), dict(top_p=1.0, min_p=0.0)):
            e, k = NM.weights(x, 0.7, top_k, **kw)
            assert (e == e0).all() and (k == k0).all()
            assert (NM.sample(x, 4, 11, 0.7, top_k, **kw) == SM.sample(x, 4, 11, 0.7, top_k)).all()
    assert (NM.sample(x, 4, 11, 0, None, top_p=0.1, min_p=0.9) == x.argmax(1)).all()          # greedy ignores both


def test_case_table_is_away_from_every_decision_boundary():
    """the condition under which the GPU test may demand an exactly equal kept set: a last-bit difference of an fp64 exp moves
    G / S1 and e / min_p by ~1e-16 relative (~1e-12 once summed over a row), never by 1e-8"""
    worst_g = worst_m = np.inf
    for i, (V, M, temperature, top_k, top_p, min_p) in enumerate(NM.CASES):
        mg, mm = NM.margins(NM.case_logits(i), temperature, top_k, top_p, min_p)
        assert (mg >= NM.MARGIN).all() and (mm >= NM.MARGIN).all(), (i, mg.min(), mm.min())
        worst_g, worst_m = min(worst_g, mg.min()), min(worst_m, mm.min())
    print(f"worst margins: top-p {worst_g:.2e}, min-p {worst_m:.2e}")


# ---------------------------------------------------------------------------------------------------------- generate() arguments
def _lm():
    import drakegpt_amd as D
    return D.TransformerLM(80, 32, 8, 4, 1, 0.0).eval()


@pytest.mark.parametrize("kw", [dict(top_p=0), dict(top_p=0.0), dict(top_p=-0.1), dict(top_p=1.0001), dict(top_p=float("nan")),
                                dict(top_p=float("inf")), dict(top_p=True), dict(top_p="0.9x"), dict(min_p=-1e-9), dict(min_p=1.5),
                                dict(min_p=float("nan")), dict(min_p=False), dict(min_p=True), dict(top_p=0.9, min_p=2)])
@pytest.mark.parametrize("cls", ["TransformerLM", "BigramLM"])
@pytest.mark.parametrize("sampler", ["host", "device"])
def test_generate_rejects_bad_top_p_and_min_p_before_the_device(cls, sampler, kw):
    import drakegpt_amd as D
    m = _lm() if cls == "TransformerLM" else D.BigramLM(80)
    idx = torch.zeros((1, 1), dtype=torch.long)              # a CPU tensor: a valid call would fail with "must be on the GPU"
    with pytest.raises(ValueError):
        m.generate(idx, 2, sampler=sampler, **kw)


@pytest.mark.parametrize("kw", [dict(top_p=0.9), dict(top_p=1), dict(top_p=1e-9), dict(min_p=0), dict(min_p=1), dict(top_p=0.5, min_p=0.05,
                                                                                                                 top_k=7)])
@pytest.mark.parametrize("sampler", ["host", "device"])
def test_valid_top_p_and_min_p_reach_the_gpu_check(sampler, kw):
    with pytest.raises(RuntimeError, match="GPU"):
        _lm().generate(torch.zeros((1, 1), dtype=torch.long), 2, sampler=sampler, **kw)


def test_check_functions():
    import inspect
    from drakegpt_amd.model import check_nucleus_args, check_sampling_args, MODEL_CLASSES
    assert check_nucleus_args(None, None) == (None, None)
    assert check_nucleus_args(1, 0) == (1.0, 0.0)
    assert check_nucleus_args(np.float32(0.5), None) == (0.5, None)
    assert list(inspect.signature(check_sampling_args).parameters) == ["sampler", "temperature", "top_k", "vocab_size"]
    assert check_sampling_args("device", 0, 500, 80) == (0.0, 80)
    for cls in MODEL_CLASSES.values():                                   # all six models
        p = inspect.signature(cls.generate).parameters
        assert p["top_p"].default is None and p["min_p"].default is None
        assert p["top_p"].kind is p["min_p"].kind is inspect.Parameter.KEYWORD_ONLY


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def test_parameter_block_packing():
    from drakegpt_amd import ops
    cpu = torch.device("cpu")
    two = ops.new_sample_params(0.5, 40, cpu)
    assert two.dtype == torch.int32 and two.tolist() == [_bits(2.0), 40]
    assert ops.new_sample_params(0, None, cpu).tolist() == [0, 0]
    assert ops.new_sample_params(0.5, 40, cpu, top_p=None, min_p=None).tolist() == two.tolist()
    four = ops.new_sample_params(0.5, 40, cpu, top_p=0.9, min_p=0.05)
    assert four.dtype == torch.int32 and four.tolist() == [_bits(2.0), 40, _bits(0.9), _bits(0.05)]
    assert four.tolist()[2:] == [0x3F666666, 0x3D4CCCCD]                 # fp32(0.9), fp32(0.05)
    assert ops.new_sample_params(1.0, None, cpu, top_p=0.9).tolist() == [_bits(1.0), 0, _bits(0.9), 0]
    assert ops.new_sample_params(1.0, None, cpu, min_p=0.1).tolist() == [_bits(1.0), 0, _bits(1.0), _bits(0.1)]
    assert ops.new_sample_params(1.0, None, cpu, top_p=1.0, min_p=0.0).tolist() == [_bits(1.0), 0, _bits(1.0), 0]


def test_entry_point_is_bound():
    from drakegpt_amd import _lib
    assert len(_lib.SIGNATURES["dg_sample_rows_nucleus"]) == len(_lib.SIGNATURES["dg_sample_rows"]) == 11
    assert hasattr(_lib.lib, "dg_sample_rows_nucleus")
    # argument errors are reported, not launched: no logits, no outputs
    assert _lib.lib.dg_sample_rows_nucleus(None, 80, 1, 80, None, None, None, 0, None, 0, None) == -1


def test_tool_parsers_have_the_flags():
    from drakegpt_amd import train
    a = train.build_parser().parse_args([])
    assert (a.top_p, a.min_p) == (None, None)
    a = train.build_parser().parse_args(["--top-p", "0.9", "--min-p", "0.05", "--top-k", "40"])
    assert (a.top_k, a.top_p, a.min_p) == (40, 0.9, 0.05)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "generate_bench.py")).read()
    assert '"--top-p"' in src and '"--min-p"' in src
