"""CPU: the controls of generate() (repetition / presence / frequency penalties, logit_bias, stop tokens) are validated in plain
Python before anything touches a device; the control block's packing; both new entries are declared, bound and refuse bad
arguments without a launch; the restatement (tests/control_model.py) against the torch statement of HF's processors."""
import inspect
import os
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_model as CM  # noqa: E402
import nucleus_model as NM  # noqa: E402

NAN, INF = float("nan"), float("inf")


def _lm():
    import drakegpt_amd as D
    return D.TransformerLM(80, 32, 8, 4, 1, 0.0).eval()


BAD = [
    dict(repetition_penalty=0), dict(repetition_penalty=-1.0), dict(repetition_penalty=NAN), dict(repetition_penalty=INF),
    dict(repetition_penalty=True), dict(repetition_penalty="1.2x"), dict(repetition_penalty=None),
    dict(presence_penalty=NAN), dict(presence_penalty=INF), dict(presence_penalty=True), dict(presence_penalty="a"),
    dict(frequency_penalty=NAN), dict(frequency_penalty=-INF), dict(frequency_penalty=False),
    dict(logit_bias={80: 1.0}), dict(logit_bias={-1: 1.0}), dict(logit_bias={3: NAN}), dict(logit_bias={3: INF}),
    dict(logit_bias={3: True}), dict(logit_bias={True: 1.0}), dict(logit_bias={1.5: 1.0}), dict(logit_bias={3: "x"}),
    dict(logit_bias=[0.0] * 79), dict(logit_bias=[0.0] * 81), dict(logit_bias=[NAN] + [0.0] * 79), dict(logit_bias=[INF] + [0.0] * 79),
    dict(logit_bias=[-INF] * 80), dict(logit_bias={j: -INF for j in range(80)}), dict(logit_bias=torch.zeros(2, 40)),
    dict(logit_bias=1.0), dict(logit_bias="ban"),
    dict(stop_tokens=80), dict(stop_tokens=-1), dict(stop_tokens=True), dict(stop_tokens=[1, 1]), dict(stop_tokens=[]),
    dict(stop_tokens=list(range(9))), dict(stop_tokens=[1.5]), dict(stop_tokens=[True]), dict(stop_tokens=2.0), dict(stop_tokens="3"),
    dict(pad_token=3), dict(stop_tokens=3, pad_token=80), dict(stop_tokens=3, pad_token=-1), dict(stop_tokens=3, pad_token=True),
    dict(stop_tokens=3, pad_token=1.0),
    dict(stop_poll=0), dict(stop_poll=-4), dict(stop_poll=1.5), dict(stop_poll=True), dict(stop_poll=None),
    dict(stop_tokens=3, stop_poll=0),
]


@pytest.mark.parametrize("kw", BAD, ids=[str(i) for i in range(len(BAD))])
@pytest.mark.parametrize("cls", ["TransformerLM", "BigramLM"])
@pytest.mark.parametrize("sampler", ["host", "device"])
def test_generate_rejects_bad_controls_before_the_device(cls, sampler, kw):
    import drakegpt_amd as D
    m = _lm() if cls == "TransformerLM" else D.BigramLM(80)
    idx = torch.zeros((1, 1), dtype=torch.long)              # a CPU tensor: a valid call would fail with "must be on the GPU"
    with pytest.raises(ValueError):
        m.generate(idx, 2, sampler=sampler, **kw)


GOOD = [
    dict(repetition_penalty=1.3), dict(repetition_penalty=0.5), dict(repetition_penalty=np.float32(1.25)), dict(presence_penalty=-0.5),
    dict(frequency_penalty=2), dict(logit_bias={3: -INF, 79: 2.5}), dict(logit_bias=[-INF] * 79 + [0.0]),
    dict(logit_bias=torch.zeros(80)), dict(logit_bias=np.zeros(80)), dict(stop_tokens=3), dict(stop_tokens=np.int64(3)),
    dict(stop_tokens=[0, 79, 5]), dict(stop_tokens=list(range(8)), pad_token=79, stop_poll=1),
    dict(repetition_penalty=1.1, presence_penalty=0.2, frequency_penalty=0.1, logit_bias={1: -INF}, stop_tokens=(4, 5), pad_token=0,
         stop_poll=7, top_p=0.9, top_k=10),
]


@pytest.mark.parametrize("kw", GOOD, ids=[str(i) for i in range(len(GOOD))])
@pytest.mark.parametrize("cls", ["TransformerLM", "BigramLM"])
@pytest.mark.parametrize("sampler", ["host", "device"])
def test_valid_controls_reach_the_gpu_check(cls, sampler, kw):
    import drakegpt_amd as D
    m = _lm() if cls == "TransformerLM" else D.BigramLM(80)
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(torch.zeros((1, 1), dtype=torch.long), 2, sampler=sampler, **kw)


def test_check_control_args():
    from drakegpt_amd.model import check_control_args, check_sampling_args
    assert check_control_args(1.0, 0.0, 0.0, None, None, None, 64, 80) is None
    assert check_control_args(1, 0, 0, None, None, None, 1, 80) is None
    c = check_control_args(1.3, 0.5, 0.25, {3: float("-inf"), 7: 2.0}, 5, None, 64, 80)
    assert (c["rep"], c["presence"], c["frequency"], c["stop"], c["pad"], c["poll"]) == (1.3, 0.5, 0.25, (5,), 5, 64)
    b = c["bias"]
    assert b.dtype == torch.float32 and b.device.type == "cpu" and b.shape == (80,)
    assert b[3] == float("-inf") and b[7] == 2.0 and int((b != 0).sum()) == 2
    c = check_control_args(1.0, 0.0, 0.0, None, [4, 9], 0, 3, 80)
    assert c["stop"] == (4, 9) and c["pad"] == 0 and c["bias"] is None and c["poll"] == 3
    assert check_control_args(1.0, 0.0, 0.0, [0.0] * 80, None, None, 64, 80)["bias"].tolist() == [0.0] * 80
    assert list(inspect.signature(check_sampling_args).parameters) == ["sampler", "temperature", "top_k", "vocab_size"]


def test_all_six_generate_signatures():
    from drakegpt_amd.model import MODEL_CLASSES
    want = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, stop_tokens=None,
                pad_token=None, stop_poll=64)
    assert len(MODEL_CLASSES) == 6
    for cls in MODEL_CLASSES.values():
        p = inspect.signature(cls.generate).parameters
        for name, default in want.items():
            assert p[name].kind is inspect.Parameter.KEYWORD_ONLY, (cls, name)
            assert p[name].default == default and type(p[name].default) is type(default), (cls, name)


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def test_control_block_packing():
    from drakegpt_amd import ops
    cpu = torch.device("cpu")
    off = ops.new_sample_control(device=cpu)
    assert off.dtype == torch.int32 and off.tolist() == [_bits(1.0), _bits(1.0), 0, 0, 0, 0, 0, 0] + [-1] * 8
    c = ops.new_sample_control(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=-0.25, stop_tokens=(7, 3), use_bias=True,
                               device=cpu)
    assert c.tolist() == [_bits(1.0 / 1.3), _bits(1.3), _bits(0.5), _bits(-0.25), 1, 2, 7, 0, 7, 3] + [-1] * 6
    assert c.tolist()[:2] == [0x3F44EC4F, 0x3FA66666]                    # fp32(1 / 1.3), fp32(1.3)
    # inv_rep is the double quotient rounded once, which numpy restates
    assert c.tolist()[0] == int(np.float32(1.0 / 1.3).view(np.int32))
    c = ops.new_sample_control(stop_tokens=list(range(10, 18)), pad_token=79, device=cpu)
    assert c.tolist() == [_bits(1.0), _bits(1.0), 0, 0, 0, 8, 79, 0] + list(range(10, 18))
    assert ops.SAMPLE_MAX_STOP == 8
    with pytest.raises(ValueError):
        ops.new_sample_control(stop_tokens=list(range(9)), device=cpu)
    # new_sample_params is untouched
    assert ops.new_sample_params(0.5, 40, cpu).tolist() == [_bits(2.0), 40]


def test_the_request_picks_the_parameter_block():
    """which block, and so which kernel entry, a generate() call gets: one assertion per row of the table (None: ops.softmax_rows;
    two words: dg_sample_rows; four: dg_sample_rows_nucleus, or dg_sample_rows_control where the operands go with it)"""
    from drakegpt_amd.model import Sampling
    cpu = torch.device("cpu")

    def block(sampler, graph=False, **kw):
        args = dict(temperature=1.0, top_k=None, seed=None, top_p=None, min_p=None, repetition_penalty=1.0, presence_penalty=0.0,
                    frequency_penalty=0.0, logit_bias=None, stop_tokens=None, pad_token=None, stop_poll=64)
        assert set(kw) <= set(args)
        p = Sampling.checked(80, None, sampler, *dict(args, **kw).values()).params(cpu, graph)
        return None if p is None else p.tolist()

    one, off = _bits(1.0), [_bits(1.0), 0]                     # top_p 1.0 and min_p 0.0: the filters filled in as "off"
    # host; temperature 1, no top_k / top_p / min_p; no penalty or bias (stop tokens alone count as none): no block
    assert block("host") is None and block("host", stop_tokens=[3, 4], pad_token=0) is None
    # host; temperature or top_k only: two words
    assert block("host", temperature=0.5) == [_bits(2.0), 0] and block("host", top_k=7, stop_tokens=3) == [one, 7]
    # host; a top_p or a min_p: four words
    assert block("host", top_p=0.9) == [one, 0, _bits(0.9), 0] and block("host", temperature=0.5, min_p=0.1) == [_bits(2.0), 0, one, _bits(0.1)]
    # host; a penalty or a bias: four words, filters filled with 1.0 / 0.0
    assert block("host", repetition_penalty=1.3) == [one, 0] + off and block("host", top_k=5, logit_bias={3: -INF}) == [one, 5] + off
    # device, eager, no controls: two words, or four with a top_p / min_p
    assert block("device") == [one, 0] and block("device", top_k=9, min_p=0.2) == [one, 9, one, _bits(0.2)]
    # device, eager, any control (a stop token alone included): four words
    assert block("device", stop_tokens=3) == [one, 0] + off and block("device", frequency_penalty=0.5, top_p=0.5) == [one, 0, _bits(0.5), 0]
    # device, graph: always four words
    assert block("device", graph=True) == [one, 0] + off and block("device", graph=True, temperature=0.0, top_k=3) == [0, 3] + off


A = 0x10000          # a made-up aligned address: nothing is dereferenced on the host, and nothing may be launched


def test_entries_are_bound_declared_and_refuse_bad_arguments():
    from drakegpt_amd import _lib
    lib = _lib.lib
    assert lib.dg_version() == 21 and _lib.ABI_VERSION == 21
    assert len(_lib.SIGNATURES["dg_sample_rows_control"]) == 16 and len(_lib.SIGNATURES["dg_token_counts"]) == 9
    assert len(_lib.SIGNATURES["dg_sample_rows_nucleus"]) == len(_lib.SIGNATURES["dg_sample_rows"]) == 11
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "drakegpt_hip.h")).read()
    assert "int dg_sample_rows_control(" in hdr and "int dg_token_counts(" in hdr and "#define DG_SAMPLE_MAX_STOP 8" in hdr
    assert "#define DG_ABI_VERSION 21" in hdr
    f = lib.dg_sample_rows_control
    #           logits ldl M  V   state params ids ld_ids probs ldp control bias counts ldc lengths stream
    ok = dict(logits=A, ldl=80, M=1, V=80, state=A, params=A, ids=A, ld_ids=8, probs=None, ldp=0, control=A, bias=None, counts=A,
              ldc=80, lengths=A)

    def call(**over):
        a = dict(ok, **over)
        return f(a["logits"], a["ldl"], a["M"], a["V"], a["state"], a["params"], a["ids"], a["ld_ids"], a["probs"], a["ldp"],
                 a["control"], a["bias"], a["counts"], a["ldc"], a["lengths"], None)

    bad = [dict(control=None), dict(ldc=79), dict(lengths=A, ids=None, probs=A, ldp=80), dict(lengths=A, ld_ids=0),
           # everything dg_sample_rows_nucleus refuses
           dict(logits=None), dict(params=None), dict(M=0), dict(V=0), dict(V=(1 << 20) + 1, ldl=1 << 21, ldc=1 << 21), dict(ldl=79),
           dict(ld_ids=-1), dict(ids=None, lengths=None), dict(state=None), dict(probs=A, ldp=79)]
    for over in bad:
        assert call(**over) == -1, over
    g = lib.dg_token_counts
    #        ids ld_ids M  n  V  counts ldc accumulate stream
    good = dict(ids=A, ld_ids=8, M=1, n=5, V=80, counts=A, ldc=80, accumulate=0)
    for over in (dict(ids=None), dict(counts=None), dict(M=0), dict(n=-1), dict(n=9), dict(V=0), dict(ldc=79)):
        a = dict(good, **over)
        assert g(a["ids"], a["ld_ids"], a["M"], a["n"], a["V"], a["counts"], a["ldc"], a["accumulate"], None) == -1, over


def test_ops_refuse_controls_without_a_block():
    from drakegpt_amd import ops
    with pytest.raises(RuntimeError, match="GPU"):
        ops.token_counts(torch.zeros((1, 4), dtype=torch.long), 4, 80)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sample_rows(torch.zeros((1, 80)), seed=1, L=0, control=ops.new_sample_control(device="cpu"))


def test_adjust_agrees_with_the_hf_processors():
    """RepetitionPenaltyLogitsProcessor: where(x > 0, x / r, x * r) on the seen tokens; then the two subtractions.  x * fp32(1 / r)
    is within one rounding of x / r: 1e-6 relative has a decade to spare over 2 * 2^-24."""
    g = np.random.default_rng(0)
    x = (g.standard_normal((32, 500)) * 4).astype(np.float32)
    counts = CM.COUNT_VALUES[g.integers(0, 6, size=x.shape)]
    for rep, presence, frequency in ((1.3, 0.0, 0.0), (0.7, 0.5, 0.25), (1.0, -0.5, 0.1), (2.5, 0.0, 1.0)):
        y = CM.adjust(x, counts, rep, presence, frequency)
        xt, ct = torch.from_numpy(x).double(), torch.from_numpy(counts)
        y1 = torch.where(ct > 0, torch.where(xt > 0, xt / rep, xt * rep), xt)
        ref = y1 - presence * (ct > 0) - frequency * ct
        # relative to the largest term: a difference of fp32 numbers that cancels (logit 0.5003 / presence 0.5) has no relative
        # accuracy of its own, in HF's own fp32 arithmetic as little as here (measured: 7e-5 of the result for either)
        scale = np.maximum(np.abs(y1.numpy()), np.maximum(abs(presence), np.abs(frequency * counts)))
        err = np.abs(y - ref.numpy())
        print(f"rep {rep}: max error / largest term {np.max(err / np.maximum(scale, 1e-30)):.2e}")
        assert (err <= 1e-6 * scale).all()
        if presence == 0 and frequency == 0:                        # the repetition penalty alone: relative to the result itself
            assert (err <= 1e-6 * np.abs(ref.numpy())).all()
    # off is the identity, bit for bit; -inf bias bans; unseen tokens are untouched by the penalties
    assert (CM.adjust(x, counts).view(np.int32) == x.view(np.int32)).all()
    b = np.zeros(500, dtype=np.float32)
    b[7] = -np.inf
    y = CM.adjust(x, counts, 1.3, 0.5, 0.25, b)
    assert np.isneginf(y[:, 7]).all() and (y[counts == 0][:] == (x + b)[counts == 0]).all()


def test_control_case_table_is_away_from_every_decision_boundary():
    for i, (V, M, temperature, top_k, top_p, min_p, rep, presence, frequency, _) in enumerate(CM.CASES):
        x, counts, bias = CM.case_inputs(i)
        assert x.shape == counts.shape == (M, V) and set(np.unique(counts)) <= {0, 1, 2, 7} and np.isneginf(bias).sum() == 4
        mg, mm = CM.margins(x, counts, rep, presence, frequency, bias, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p)
        assert (mg >= NM.MARGIN).all() and (mm >= NM.MARGIN).all(), (i, mg.min(), mm.min())


def test_restatement_generation_loop_and_stop_rule():
    V = 16
    table = (np.random.default_rng(4).standard_normal((V, V)) * 2).astype(np.float32)

    def logits_fn(ids):
        return table[ids[:, -1]]

    prompt = np.array([[1, 2], [3, 4], [5, 6]])
    plain = CM.generate(logits_fn, prompt, 30, V, seed=9)
    assert plain.shape == (3, 32)
    # a huge frequency penalty with greedy decoding never repeats a token while fresh ones are left
    g = CM.generate(logits_fn, prompt, V - 2, V, seed=9, frequency=1e4, temperature=0)
    assert all(len(set(r.tolist())) == V for r in g)
    banned = CM.generate(logits_fn, prompt, 30, V, seed=9, bias=np.where(np.arange(V) == 7, -np.inf, 0).astype(np.float32))
    assert not (banned[:, 2:] == 7).any()
    stop = (int(plain[0, 5]), int(plain[1, 11]))
    s = CM.generate(logits_fn, prompt, 30, V, seed=9, stop=stop, pad=0)
    assert (s == CM.apply_stop(plain, 2, stop, 0)).all()


def test_train_parser_has_the_flags_and_run_args_ignores_them():
    from drakegpt_amd import train
    a = train.build_parser().parse_args([])
    assert (a.repetition_penalty, a.presence_penalty, a.frequency_penalty, a.stop_token) == (1.0, 0.0, 0.0, None)
    b = train.build_parser().parse_args(["--repetition-penalty", "1.3", "--presence-penalty", "0.5", "--frequency-penalty", "0.25",
                                         "--stop-token", "3", "--stop-token", "7"])
    assert (b.repetition_penalty, b.presence_penalty, b.frequency_penalty, b.stop_token) == (1.3, 0.5, 0.25, [3, 7])
    assert train.run_args(a, 1, 1) == train.run_args(b, 1, 1)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "generate_bench.py")).read()
    assert '"--repetition-penalty"' in src and '"--presence-penalty"' in src and '"--frequency-penalty"' in src
