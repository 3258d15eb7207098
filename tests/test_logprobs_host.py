"""CPU: the numpy restatement of dg_token_logprobs (tests/logprob_model.py) against torch, the argument checks, best_of's choice,
the trimming of Generation -- and the comparison helper of the GPU tests against four planted defects: a comparison that cannot
fail shows nothing, so each defect must make logprob_model.compare fail on a case of the GPU test's own table."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_model as LM  # noqa: E402

CASES = LM.case_table()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_against_torch_log_softmax(case, bf16):
    """|lp - log_softmax_fp64| <= 2^-23 max(|lp|, 1): one fp32 rounding of x_j - m* plus one of the result; -inf and NaN alike;
    ranks and top ids equal a stable descending argsort exactly"""
    _, V, M, kind, seed = case
    full, tok = LM.make_case(V, M, kind, seed, bf16)
    assert np.isnan(full[:, V:]).all()                                     # the pad columns must never be read
    lp, rank, top_ids, top_lp = LM.token_logprobs(full, V, tok, top_n=20)
    x = torch.from_numpy(full[:, :V]).double()
    ref = torch.log_softmax(x, 1).numpy()
    t = np.clip(tok, 0, V - 1)
    rows = np.arange(full.shape[0])
    r = ref[rows, t]
    assert np.array_equal(np.isnan(lp), np.isnan(r)) and np.array_equal(np.isneginf(lp), np.isneginf(r))
    ok = np.isfinite(r)
    assert (np.abs(lp[ok].astype(np.float64) - r[ok]) <= 2.0 ** -23 * np.maximum(np.abs(r[ok]), 1)).all()
    for m in rows:
        order = np.argsort(-full[m, :V].astype(np.float64), kind="stable")
        if np.isnan(r[m]):                                                 # the all--inf row: every entry ties
            assert rank[m] == t[m] and (top_ids[m] == -1).all()
            continue
        assert rank[m] == int(np.flatnonzero(order == t[m])[0])
        best = order[full[m, order] > -np.inf][:20]
        assert np.array_equal(top_ids[m, :best.size], best) and (top_ids[m, best.size:] == -1).all()
        got = top_lp[m, :best.size].astype(np.float64)
        assert (np.abs(got - ref[m, best]) <= 2.0 ** -23 * np.maximum(np.abs(ref[m, best]), 1)).all()
        assert np.isneginf(top_lp[m, best.size:]).all()


def test_fixed_order_sum_is_the_kernels_order_not_numpys():
    """the order matters: on terms of very different size the fixed order and a plain sum differ in the last bits"""
    g = np.random.default_rng(0)
    e = np.exp(g.standard_normal((4, 50257)) * 8)
    Z = LM.fixed_order_sum(e)
    assert np.allclose(Z, e.sum(1), rtol=1e-12) and (Z != e.sum(1)).any()
    one = np.zeros((1, 300))
    one[0, 299] = 3.0
    assert LM.fixed_order_sum(one)[0] == 3.0 and LM.threads_of(8192) == 256 and LM.threads_of(8193) == 1024


# ------------------------------------------------------------------------------------------------------------------ planted defects
def _find(kind, V):
    return next(c for c in CASES if c[3] == kind and c[1] == V)


def _pair(case, defect, **kw):
    _, V, M, kind, seed = case
    full, tok = LM.make_case(V, M, kind, seed)
    return LM.token_logprobs(full, V, tok, **kw), LM.token_logprobs(full, V, tok, defect=defect, **kw)


def test_compare_accepts_the_restatement_itself_and_a_last_bit():
    good, _ = _pair(_find("randn30", 4099), None, top_n=5)
    assert LM.compare(good, good) == []
    lp = good[0].copy()
    lp.view(np.int32)[0] += 1                                              # one ulp in one of 3 entries: beyond the 0.1 % share
    assert LM.compare((lp,) + good[1:], good)
    big = np.linspace(-9, -1, 5000).astype(np.float32)
    off = big.copy()
    off.view(np.int32)[:5] += 1
    assert LM.lp_mismatch(off, big) is None                                # 0.1 % of 5000, one ulp each
    off.view(np.int32)[5] += 1
    assert LM.lp_mismatch(off, big) is not None
    two = big.copy()
    two.view(np.int32)[0] += 2
    assert LM.lp_mismatch(two, big) is not None                            # two ulps, however rare


def test_compare_refuses_log_of_p():
    """log(p) in the place of x - m* - log Z: the dominated token's p underflows in fp32 and its lp becomes -inf"""
    good, bad = _pair(_find("special", 257), "logp", top_n=5)
    assert np.isfinite(good[0][2]) and abs(good[0][2] + 200) < 10 and np.isneginf(bad[0][2])
    assert any(w.startswith("lp") for w in LM.compare(bad, good))


def test_compare_refuses_a_reversed_tie_order():
    good, bad = _pair(_find("quant4", 257), "tie_reversed", top_n=5)
    assert np.array_equal(good[0], bad[0]) and np.array_equal(good[1], bad[1])          # only the top ids move
    assert LM.compare(bad, good) == ["top_ids: differs at " + str(np.argwhere(bad[2] != good[2])[:3].tolist())]


def test_compare_refuses_a_rank_that_counts_greater_or_equal():
    for kind in ("randn1", "quant4"):
        good, bad = _pair(_find(kind, 80), "rank_ge")
        assert (bad[1] > good[1]).all()
        assert any(w.startswith("rank") for w in LM.compare(bad, good))


def test_compare_refuses_an_unscored_stop_token():
    """a row with lengths[m] = L + 1 drew its stop token AT L: it is scored; the defect leaves its sentinel in place"""
    full, _ = LM.make_case(65, 3, "randn1", 21)
    tokens = np.random.default_rng(21).integers(0, 65, size=(3, 8)).astype(np.int64)
    L, lengths = 5, [0, 6, 3]

    def run(defect):
        out = (np.full((3, 8), 7.5, np.float32), np.full((3, 8), -5, np.int32), np.full((3, 8, 20), -9, np.int32),
               np.full((3, 8, 20), 2.5, np.float32))
        return LM.token_logprobs(full, 65, tokens, top_n=2, L=L, lengths=lengths, outputs=out, defect=defect)

    good, bad = run(None), run("stop_unscored")
    assert lengths[1] == L + 1 and good[0][1, L] != 7.5 and bad[0][1, L] == 7.5
    assert good[0][2, L] == 7.5 and good[0][0, L] != 7.5                    # finished earlier: skipped; running: scored
    assert (np.delete(good[0], L, axis=1) == 7.5).all()                     # nothing but column L
    assert len(LM.compare(bad, good)) == 4


def test_skip_rules_of_the_restatement():
    full, _ = LM.make_case(65, 4, "randn1", 3)
    tokens = np.zeros((4, 6), dtype=np.int64)
    out = LM.token_logprobs(full, 65, tokens, L=2, lengths=[0, 2, 0, 0], spans=[[1, 9], [1, 9], [3, 9], [2, 9]],
                            outputs=LM.new_outputs((4, 6), fill_lp=9.0))
    assert [out[0][m, 2] != 9.0 for m in range(4)] == [True, False, False, True]
    same = LM.token_logprobs(full, 65, tokens, L=6, outputs=LM.new_outputs((4, 6), fill_lp=9.0))
    assert (same[0] == 9.0).all()                                          # L >= ld_tok: nothing


# ------------------------------------------------------------------------------------------------------------------ arguments
def _tiny():
    import drakegpt_amd as D
    torch.manual_seed(0)
    return D.TransformerLM(80, 32, 16, 4, 1, 0.0)


@pytest.mark.parametrize("kw", [dict(top_logprobs=21), dict(top_logprobs=-1), dict(top_logprobs=2.0), dict(top_logprobs=True),
                                dict(best_of=0), dict(best_of=1.5), dict(best_of=True), dict(best_of=2),
                                dict(best_of=2, prompt_lengths=[1, 2])])
@pytest.mark.parametrize("sampler", ["host", "device"])
def test_generate_checks_its_arguments_before_touching_a_device(kw, sampler):
    """a CPU model and CPU ids: anything that reached a kernel wrapper would raise RuntimeError, not ValueError"""
    m = _tiny()
    idx = torch.zeros((2, 3), dtype=torch.long)
    with pytest.raises(ValueError, match="top_logprobs|best_of|pad_token"):
        m.generate(idx, 4, sampler=sampler, **kw)


def test_score_checks_its_arguments_before_touching_a_device():
    m = _tiny()
    idx = torch.zeros((2, 5), dtype=torch.long)
    for kw in (dict(top_logprobs=21), dict(top_logprobs=-1), dict(prompt_lengths=[1]), dict(prompt_lengths=[0, 2]), dict(prompt_lengths=[6, 2])):
        with pytest.raises(ValueError):
            m.score(idx, **kw)
    with pytest.raises(RuntimeError, match="GPU"):                          # checked arguments: only now the device is asked for
        m.score(idx)


def test_ops_wrapper_checks_before_touching_a_device():
    from drakegpt_amd import ops
    assert ops.LOGPROBS_MAX_TOP == LM.MAX_TOP == 20
    for bad in (21, -1, 1.0, True, None):
        with pytest.raises(ValueError):
            ops.check_top_logprobs(bad)
    assert [ops.check_top_logprobs(n) for n in (0, 5, 20)] == [0, 5, 20]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.token_logprobs(torch.zeros(2, 4), torch.zeros(2, dtype=torch.long))
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "drakegpt_hip.h")).read()
    assert "#define DG_LOGPROBS_MAX_TOP 20" in hdr and "int dg_token_logprobs(" in hdr


def test_sampling_request_carries_the_new_fields():
    from drakegpt_amd.model import Sampling
    base = dict(generator=None, sampler="device", temperature=1.0, top_k=None, seed=1, top_p=None, min_p=None, repetition_penalty=1.0,
                presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, stop_tokens=None, pad_token=None, stop_poll=64)
    plain = Sampling.checked(80, **base)
    assert not plain.scored and plain.ctl is None and plain.best_of == 1     # a call without the arguments is the call it was
    assert Sampling.checked(80, **base, return_logprobs=True).scored and Sampling.checked(80, **base, top_logprobs=1).scored
    req = Sampling.checked(80, **dict(base, pad_token=7), best_of=3, prompt_lengths=[2, 1], shape=(2, 4))
    assert req.scored and req.ctl["pad"] == 7 and req.prompt_lengths == (2, 2, 2, 1, 1, 1)
    idx, done = req.enter(torch.tensor([[5, 6, 9, 9], [4, 9, 9, 9]]), 3)
    assert done is None and idx.tolist() == [[5, 6]] * 3 + [[4, 7]] * 3      # candidate c of prompt b is row 3 b + c


# ------------------------------------------------------------------------------------------------------------------ best_of, trimming
def test_best_of_selection_on_hand_made_logprobs():
    from drakegpt_amd.model import Generation, keep_best_of, select_best_of
    Z = 0.0
    lp = torch.tensor([
        # prompt 0 (length 2), candidates 0..2
        [Z, Z, -1.0, -1.0, -1.0, Z],        # mean -1 over 3 tokens
        [Z, Z, -0.5, -0.5, Z, Z],           # stopped early, mean -0.5 over 2: wins although its SUM (-1) loses to no one's
        [Z, Z, -0.5, -0.5, -0.5, -0.5],     # mean -0.5 over 4: a tie with candidate 1 -> the lowest c stays
        # prompt 1 (length 3)
        [Z, Z, Z, -2.0, -2.0, -2.0],
        [Z, Z, Z, -3.0, Z, Z],              # one token
        [Z, Z, Z, -1.0, -2.5, Z],           # mean -1.75: wins
    ])
    lengths = torch.tensor([5, 4, 6, 6, 4, 5])
    first = (2, 2, 2, 3, 3, 3)
    assert select_best_of(lp, lengths, first, 3).tolist() == [1, 5]
    ids = torch.arange(36).view(6, 6)
    gen = Generation(ids, lengths, lp, torch.full((6, 6, 2), -1, dtype=torch.int32), torch.full((6, 6, 2), -math.inf))
    best = keep_best_of(gen, first, 3, pad=0)
    assert best.ids.shape == (2, 5) and best.lengths.tolist() == [4, 5]       # trimmed again, to the longest KEPT row
    assert torch.equal(best.ids, ids[[1, 5], :5]) and torch.equal(best.logprobs, lp[[1, 5], :5])
    assert best.top_ids.shape == (2, 5, 2)
    # a candidate that generated nothing never wins over one that did; all empty: candidate 0
    assert select_best_of(torch.zeros(2, 3), torch.tensor([2, 3]), (2, 2), 2).tolist() == [1]
    assert select_best_of(torch.zeros(2, 3), torch.tensor([2, 2]), (2, 2), 2).tolist() == [0]
    assert select_best_of(torch.tensor([[0.0, -1.0], [0.0, -1.0]]), torch.tensor([2, 2]), (1, 1), 2).tolist() == [0]


def test_generation_is_trimmed_and_zero_filled():
    from drakegpt_amd.model import make_generation, new_score_buffers
    lp, ti, tl = new_score_buffers(2, 8, "cpu")
    assert (lp == 0).all() and (ti == -1).all() and torch.isneginf(tl).all() and ti.shape == (2, 8, 20) and ti.dtype == torch.int32
    ids = torch.arange(16).view(2, 8)
    lp[0, 2:5], lp[1, 2:4] = -1.0, -2.0
    ti[0, 2:5, :3], tl[0, 2:5, :3] = 4, -0.5
    gen = make_generation(ids, torch.tensor([5, 4], dtype=torch.int32), 8, lp, ti, tl, 3)
    assert gen.ids.shape == (2, 5) and gen.lengths.tolist() == [5, 4] and gen.lengths.dtype == torch.int64
    assert gen.logprobs.shape == (2, 5) and gen.top_ids.shape == (2, 5, 3) and gen.top_logprobs.shape == (2, 5, 3)
    assert gen.logprobs.sum(1).tolist() == [-3.0, -4.0]                      # the log-likelihood of what each row generated
    assert gen.logprobs[1, 4] == 0 and (gen.top_ids[1] == -1).all() and (gen.top_ids[0, 2:5] == 4).all()
    run = make_generation(ids, torch.tensor([0, 4], dtype=torch.int32), 7, lp, ti, tl, 0)        # a row still running: `total`
    assert run.ids.shape == (2, 7) and run.lengths.tolist() == [7, 4] and run.top_ids.shape == (2, 7, 0)
    none = make_generation(ids, None, 6, lp, ti, tl, 1)
    assert none.ids.shape == (2, 6) and none.lengths.tolist() == [6, 6]


def test_score_helpers_on_hand_made_values():
    from drakegpt_amd.model import Score
    lp = torch.tensor([[-1.0, -3.0, 0.0], [-2.0, 0.0, 0.0]])
    rk = torch.tensor([[0, 4, -1], [1, -1, -1]], dtype=torch.int32)
    mask = torch.tensor([[True, True, False], [True, False, False]])
    sc = Score(lp, rk, torch.empty(2, 3, 0), torch.empty(2, 3, 0), mask)
    assert abs(sc.perplexity() - math.exp(2.0)) < 1e-12
    assert sc.accuracy() == pytest.approx(1 / 3) and sc.accuracy(2) == pytest.approx(2 / 3) and sc.accuracy(5) == 1.0


def test_the_oracle_keeps_the_rank_test_inside_its_cap():
    """the CPU half of the GPU rank test (tests/test_gpu_generate_logprobs.py): on LM.rank_case_ids the oracle has another logit
    within 4 e of the target's at no more than 5 % of the positions, for every e up to 1e-4 -- a hundred times what fp32 reaches"""
    from oracle import drake_ref as R
    import drakegpt_amd as D
    torch.manual_seed(42)
    m = D.TransformerLM(80, 64, 32, 4, 2, 0.0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ids = LM.rank_case_ids(80, 33)
    with torch.no_grad():
        o = R.lm_forward("TransformerLM", sd, ids[:, :32])[0].double()
    clear, rank = LM.clear_positions(o, ids[:, 1:], 1e-4)
    assert clear.float().mean().item() >= 0.95 and rank.min() >= 0 and rank.max() < 80
