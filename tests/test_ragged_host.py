"""CPU: generate(prompt_lengths=, return_lengths=) -- the argument checks (check_prompt_lengths, the pad_token rule), the request
that carries them, the six signatures, the two new library entries, and the numpy restatement tests/ragged_model.py, whose
defining property is stated on a toy model: a row of a ragged batch has the tokens of a rectangular batch made of its own prompt."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_model as CM  # noqa: E402
import ragged_model as RM  # noqa: E402

V = 80


def _lm():
    import drakegpt_amd as D
    return D.TransformerLM(V, 64, 32, 4, 2, 0.0)


# idx is (3, 6) throughout
BAD = [
    [1, 2], [1, 2, 3, 4], [], 3, object(), "123",                                 # wrong count, not a sequence of integers
    [1, 2, 2.0], [1, 2, True], [1, 2, None], [1, 2, "3"], [1.5, 2, 3],            # non-integers, bools
    [0, 2, 3], [1, 2, 7], [-1, 2, 3], [6, 6, 100],                                # out of [1, T]
    torch.tensor([1.0, 2.0, 3.0]), torch.tensor([True, True, True]), torch.tensor([[1, 2, 3]]), torch.tensor([1, 2]),
    torch.tensor([0, 1, 2]), torch.tensor([1, 2, 7]), np.array([1.0, 2.0, 3.0]),
]
GOOD = [[1, 2, 3], (6, 6, 6), [6, 1, 3], torch.tensor([1, 2, 3]), torch.tensor([4, 5, 6], dtype=torch.int32), np.array([2, 6, 1]),
        [np.int64(1), np.int32(2), 3], range(1, 4)]


@pytest.mark.parametrize("p", BAD, ids=[str(i) for i in range(len(BAD))])
def test_check_prompt_lengths_refuses(p):
    from drakegpt_amd.model import check_prompt_lengths
    with pytest.raises(ValueError):
        check_prompt_lengths(p, (3, 6))


@pytest.mark.parametrize("p", GOOD, ids=[str(i) for i in range(len(GOOD))])
def test_check_prompt_lengths_accepts(p):
    from drakegpt_amd.model import check_prompt_lengths
    got = check_prompt_lengths(p, (3, 6))
    assert isinstance(got, tuple) and all(type(x) is int for x in got)
    assert list(got) == [int(x) for x in (p.tolist() if hasattr(p, "tolist") else p)]


def test_check_prompt_lengths_none_and_shape():
    from drakegpt_amd.model import check_prompt_lengths
    assert check_prompt_lengths(None, (3, 6)) is None and check_prompt_lengths(None, ()) is None
    with pytest.raises(ValueError):
        check_prompt_lengths([1, 2, 3], (3,))
    with pytest.raises(ValueError):
        check_prompt_lengths([1, 2, 3], ())


@pytest.mark.parametrize("cls", ["TransformerLM", "BigramLM"])
@pytest.mark.parametrize("sampler", ["host", "device"])
def test_generate_checks_before_the_device(cls, sampler):
    """every refusal is a ValueError raised on a CPU idx, whose valid calls fail later with "must be on the GPU" """
    import drakegpt_amd as D
    m = _lm() if cls == "TransformerLM" else D.BigramLM(V)
    idx = torch.zeros((3, 6), dtype=torch.long)
    for p in BAD:
        with pytest.raises(ValueError):
            m.generate(idx, 2, sampler=sampler, prompt_lengths=p, pad_token=0)
    # the pad_token rule: prompt_lengths pads, so it needs a pad_token or stop_tokens ...
    with pytest.raises(ValueError, match="prompt_lengths needs"):
        m.generate(idx, 2, sampler=sampler, prompt_lengths=[1, 2, 3])
    with pytest.raises(ValueError, match="prompt_lengths needs"):
        m.generate(idx, 2, sampler=sampler, prompt_lengths=[1, 2, 3], repetition_penalty=1.3)
    # ... and pad_token alone is still refused
    with pytest.raises(ValueError, match="pad_token needs"):
        m.generate(idx, 2, sampler=sampler, pad_token=3)
    with pytest.raises(ValueError, match="pad_token needs"):
        m.generate(idx, 2, sampler=sampler, pad_token=3, return_lengths=True)
    with pytest.raises(ValueError):
        m.generate(idx, 2, sampler=sampler, prompt_lengths=[1, 2, 3], pad_token=V)
    for kw in (dict(pad_token=3), dict(stop_tokens=5), dict(stop_tokens=[5, 6], pad_token=0), dict(pad_token=0, repetition_penalty=1.2)):
        for p in GOOD[:4]:
            with pytest.raises(RuntimeError, match="GPU"):
                m.generate(idx, 2, sampler=sampler, prompt_lengths=p, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(idx, 2, sampler=sampler, return_lengths=True)


def test_control_dict_of_a_ragged_call():
    from drakegpt_amd.model import check_control_args
    assert check_control_args(1.0, 0.0, 0.0, None, None, None, 64, V) is None
    with pytest.raises(ValueError):
        check_control_args(1.0, 0.0, 0.0, None, None, 3, 64, V)
    with pytest.raises(ValueError):
        check_control_args(1.0, 0.0, 0.0, None, None, None, 64, V, ragged=True)
    c = check_control_args(1.0, 0.0, 0.0, None, None, 3, 64, V, ragged=True)                 # nothing adjusts, and still a dict
    assert c["pad"] == 3 and c["stop"] == () and c["adjust"] is False and c["bias"] is None
    c = check_control_args(1.0, 0.0, 0.0, None, [7, 9], None, 64, V, ragged=True)
    assert c["pad"] == 7 and c["stop"] == (7, 9)


def test_the_request_carries_the_lengths():
    from drakegpt_amd.model import Sampling
    args = (V, None, "device", 1.0, None, 5, None, None, 1.0, 0.0, 0.0, None, None)
    plain = Sampling.checked(*args, None, 64)
    assert plain.prompt_lengths is None and not plain.ragged and plain.return_lengths is False and plain.ctl is None
    assert plain.span(6, 10) == (6, 16)
    idx = torch.arange(18).view(3, 6)
    assert plain.enter(idx, 10)[0] is idx and plain.enter(idx, 10)[1] is None
    req = Sampling.checked(*args, 79, 64, torch.tensor([2, 5, 3]), (3, 6), True)
    assert req.prompt_lengths == (2, 5, 3) and req.ragged and req.return_lengths is True and req.ctl["pad"] == 79 and req.poll == 0
    assert req.span(6, 10) == (2, 15)
    assert req.params(torch.device("cpu")).numel() == 4                   # the device sampler's control entry: four words
    padded, done = req.enter(idx, 10)
    assert done is None and idx[0, 2] == 2                                # the caller's tensor is not written
    assert padded.tolist() == [[0, 1, 79, 79, 79], [6, 7, 8, 9, 10], [12, 13, 14, 79, 79]]
    # no new tokens: the padded prompts and their lengths
    out, n = req.enter(idx, 0)[1]
    assert out.tolist() == padded.tolist() and n.tolist() == [2, 5, 3] and n.dtype == torch.int64
    assert Sampling.checked(*args, 79, 64, [2, 5, 3], (3, 6)).enter(idx, 0)[1].tolist() == padded.tolist()


def test_trim_to_longest_with_lengths():
    from drakegpt_amd.model import trim_to_longest
    ids = torch.arange(40).view(4, 10)
    assert trim_to_longest(ids, None, 7).shape == (4, 7)
    out, n = trim_to_longest(ids, None, 7, True)
    assert out.shape == (4, 7) and n.tolist() == [7] * 4 and n.dtype == torch.int64
    out, n = trim_to_longest(ids, torch.tensor([3, 0, 5, 0], dtype=torch.int32), 8, True)
    assert out.shape == (4, 8) and n.tolist() == [3, 8, 5, 8] and n.dtype == torch.int64
    assert trim_to_longest(ids, torch.tensor([3, 4, 5, 2], dtype=torch.int32), 8).shape == (4, 5)


def test_all_six_generate_signatures():
    from drakegpt_amd.model import MODEL_CLASSES
    assert len(MODEL_CLASSES) == 6
    for cls in MODEL_CLASSES.values():
        p = inspect.signature(cls.generate).parameters
        assert p["prompt_lengths"].kind is inspect.Parameter.KEYWORD_ONLY and p["prompt_lengths"].default is None, cls
        assert p["return_lengths"].kind is inspect.Parameter.KEYWORD_ONLY and p["return_lengths"].default is False, cls


def test_the_library_has_the_two_entries():
    from drakegpt_amd import _lib
    assert len(_lib.SIGNATURES["dg_sample_rows_ragged"]) == len(_lib.SIGNATURES["dg_sample_rows_control"]) + 1
    assert len(_lib.SIGNATURES["dg_token_counts_rows"]) == len(_lib.SIGNATURES["dg_token_counts"]) + 1
    assert hasattr(_lib.lib, "dg_sample_rows_ragged") and hasattr(_lib.lib, "dg_token_counts_rows")
    assert _lib.lib.dg_version() == 21                          # new entries, no signature changed


# ------------------------------------------------------------------------------------------------------------ the restatement
def toy_logits(ids):
    """fp32 [B, V] of the next position; a row's output depends on that row alone (its last three tokens and its length)"""
    ids = np.asarray(ids)
    out = np.empty((ids.shape[0], V), dtype=np.float32)
    for b, r in enumerate(ids):
        out[b] = np.random.default_rng([len(r)] + [int(t) for t in r[-3:]]).standard_normal(V) * 3
    return out


PROMPTS = [[2, 3], [5, 7, 1, 4, 9, 11, 13, 2, 6], [1, 4, 8, 3, 10], [12]]
PAD = 79
SETTINGS = [dict(), dict(temperature=0.7, top_k=20, top_p=0.9), dict(rep=1.3, presence=0.2, frequency=0.1, top_p=0.95),
            dict(temperature=0.0, frequency=2.0)]


@pytest.mark.parametrize("kw", SETTINGS, ids=[str(i) for i in range(len(SETTINGS))])
def test_a_ragged_row_is_the_row_of_a_rectangular_run_on_its_prompt(kw):
    n_new, seed = 12, 77
    prompt, p = RM.pad_prompts(PROMPTS, -5, width=11)                       # what lies in the padding is never read
    out, final = RM.generate(toy_logits, prompt, p, n_new, V, seed, pad=PAD, **kw)
    assert out.shape == (4, max(p) + n_new) and final.tolist() == [q + n_new for q in p]
    for b, q in enumerate(p):
        rect = CM.generate(toy_logits, np.tile(np.array(PROMPTS[b]), (4, 1)), n_new, V, seed, **kw)
        assert out[b, :q + n_new].tolist() == rect[b].tolist(), b               # the same seed, the same row index
        assert (out[b, q + n_new:] == PAD).all()
    # the rows do depend on their row index: the property is not vacuous
    rect = CM.generate(toy_logits, np.tile(np.array(PROMPTS[0]), (4, 1)), n_new, V, seed, **SETTINGS[0])
    assert len({str(r.tolist()) for r in rect}) == 4


def test_ragged_restatement_stop_tokens_and_equal_lengths():
    n_new, seed = 12, 78
    prompt, p = RM.pad_prompts(PROMPTS, 0)
    plain, _ = RM.generate(toy_logits, prompt, p, n_new, V, seed, pad=PAD)
    stop = (int(plain[1, p[1] + 4]), int(plain[3, p[3] + 7]))
    out, final = RM.generate(toy_logits, prompt, p, n_new, V, seed, stop=stop, pad=PAD)
    assert final[1] <= p[1] + 5 and final[3] <= p[3] + 8 and out.shape[1] == final.max()
    for b, q in enumerate(p):
        end = int(final[b])
        assert out[b, :end].tolist() == plain[b, :end].tolist() and (out[b, end:] == PAD).all()
        assert end == q + n_new or int(out[b, end - 1]) in stop
        assert not set(out[b, q:end - 1].tolist()) & set(stop)
        rect = CM.generate(toy_logits, np.tile(np.array(PROMPTS[b]), (4, 1)), n_new, V, seed, stop=stop, pad=PAD)
        assert out[b, :end].tolist() == rect[b, :end].tolist()
    # a prompt token that is a stop token ends nothing: row 1 holds 7 in its prompt
    out, final = RM.generate(toy_logits, prompt, p, 3, V, seed, stop=(7,), pad=PAD)
    assert final[1] > p[1]
    # equal lengths: control_model's loop
    rect = np.tile(np.array(PROMPTS[2]), (3, 1))
    a, final = RM.generate(toy_logits, rect, [5, 5, 5], n_new, V, seed, rep=1.2, pad=PAD)
    assert a.tolist() == CM.generate(toy_logits, rect, n_new, V, seed, rep=1.2).tolist() and final.tolist() == [17] * 3
    # no new tokens
    out, final = RM.generate(toy_logits, prompt, p, 0, V, seed, pad=PAD)
    assert out.tolist() == RM.pad_prompts(PROMPTS, PAD)[0].tolist() and final.tolist() == p
