"""GPU: dg_token_logprobs against its numpy restatement (tests/logprob_model.py), inside guard bands.

Ranks and top ids equal the restatement exactly.  The log-probabilities are bit-equal to it in all but at most 0.1 % of the
entries of an output, and those differ by one fp32 ulp (logprob_model.lp_mismatch): both sides add bit-identical fp64 terms in one
order and can differ only in the last bit of an fp64 exp or log, which moves the fp32 rounding of lp only at a rounding boundary --
an expected share of about 1e-8, so the cap is a condition, not a tolerance.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logprob_model as LM  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64                      # elements on either side of every output
TOP = LM.MAX_TOP
_SENT = {torch.float32: 12345.0, torch.int32: -77}


class Guarded:
    """an output of n elements between two guard bands that hold a known pattern"""

    def __init__(self, n, dtype, dev, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), _SENT[dtype] if fill is None else fill, dtype=dtype, device=dev)
        self.buf[:GUARD] = _SENT[dtype]
        self.buf[GUARD + n:] = _SENT[dtype]
        self.before = self.buf.cpu().numpy().copy()

    @property
    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        now = self.buf.cpu().numpy()
        return (now[:GUARD].tobytes() == self.before[:GUARD].tobytes()
                and now[GUARD + self.n:].tobytes() == self.before[GUARD + self.n:].tobytes())


def _device_logits(full, V, bf16, dev):
    """the [M, V] view of a [M, ldl] buffer whose pad columns hold NaN"""
    t = torch.from_numpy(full)
    if bf16:
        t = t.to(torch.bfloat16)
    return t.to(dev)[:, :V]


def _launch(dev, logits, tokens, *, ld_tok=0, state=None, lengths=None, spans=None, top_n=None, outs=(None,) * 4):
    from drakegpt_amd import _lib, ops
    M, V = logits.shape
    p = ops._p
    return _lib.lib.dg_token_logprobs(p(logits), ops.dt_code(logits.dtype), ops._ld(logits), M, V, p(tokens), ld_tok, p(state), p(lengths),
                                      p(spans), p(top_n), *[p(o) for o in outs], ops._stream())


def _run_flat(dev, full, V, tok, bf16, top_n, with_top=True):
    """the ld_tok == 0 form on guarded outputs -> (lp, rank, top_ids, top_lp) as numpy, the guards checked"""
    M = full.shape[0]
    x = _device_logits(full, V, bf16, dev)
    g = [Guarded(M, torch.float32, dev), Guarded(M, torch.int32, dev), Guarded(M * TOP, torch.int32, dev), Guarded(M * TOP, torch.float32, dev)]
    outs = [o.body for o in g]
    if not with_top:
        outs[2] = outs[3] = None
    n_dev = torch.tensor([top_n], dtype=torch.int32, device=dev)
    rc = _launch(dev, x, torch.from_numpy(tok).to(dev), top_n=n_dev, outs=outs)
    torch.cuda.synchronize(dev)
    assert rc == 0
    for o in g:
        assert o.guards_intact()
    return (g[0].body.cpu().numpy(), g[1].body.cpu().numpy(), g[2].body.cpu().numpy().reshape(M, TOP), g[3].body.cpu().numpy().reshape(M, TOP))


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", LM.case_table(), ids=[c[0] for c in LM.case_table()])
def test_kernel_matches_the_restatement(dev, case, bf16):
    _, V, M, kind, seed = case
    full, tok = LM.make_case(V, M, kind, seed, bf16)
    top_n = (5, 20, 1, 3)[seed % 4]
    got = _run_flat(dev, full, V, tok, bf16, top_n)
    want = LM.token_logprobs(full, V, tok, top_n=top_n)
    bad = LM.compare(got, want)
    assert not bad, bad
    if kind == "special":
        lp = got[0]
        assert (np.isneginf(lp[0]) or V == 1) and np.isnan(lp[1])
        assert np.isfinite(lp[2]) and (V == 1 or abs(lp[2] + 200) < 3 + np.log(V)), lp[2]         # dominated, not -inf
        assert V == 1 or got[1][3] == 0 and got[1][6] == 0                                          # the token at the maximum
        assert (got[2][1] == -1).all() and np.isneginf(got[3][1]).all()                             # no finite entry: no top


@pytest.mark.parametrize("top_n", [0, 1, 5, 20, 25])
@pytest.mark.parametrize("V", [3, 80, 4099])
def test_top_n_settings(dev, V, top_n):
    """0 (no selection, sentinels only), up to the clamp at 20, and top_n > V"""
    full, tok = LM.make_case(V, 3, "quant4" if V == 80 else "randn1", 5 + V)
    got = _run_flat(dev, full, V, tok, False, top_n)
    want = LM.token_logprobs(full, V, tok, top_n=top_n)
    assert not LM.compare(got, want)
    n = min(top_n, 20, V)
    assert (got[2][:, :n] >= 0).all() and (got[2][:, n:] == -1).all() and np.isneginf(got[3][:, n:]).all()


def test_outputs_are_nullable(dev):
    full, tok = LM.make_case(257, 3, "randn1", 9)
    want = LM.token_logprobs(full, 257, tok, top_n=5)
    got = _run_flat(dev, full, 257, tok, False, 5, with_top=False)
    assert not LM.compare(got[:2] + (None, None), want)
    x = _device_logits(full, 257, False, dev)
    t = torch.from_numpy(tok).to(dev)
    rk = Guarded(3, torch.int32, dev)
    assert _launch(dev, x, t, outs=(None, rk.body, None, None)) == 0
    torch.cuda.synchronize(dev)
    assert rk.guards_intact() and np.array_equal(rk.body.cpu().numpy(), want[1])


def _decode_case(dev, L, cap, lengths, spans, top_n=3, V=65, seed=21, M=None):
    """the ld_tok > 0 form on M = len(lengths) rows at position L; outputs pre-filled with a sentinel pattern"""
    from drakegpt_amd import ops
    M = len(lengths) if M is None else M
    full, _ = LM.make_case(V, M, "randn1", seed)
    g = np.random.default_rng(seed)
    tokens = g.integers(0, V, size=(M, cap)).astype(np.int64)
    x = _device_logits(full, V, False, dev)
    gs = [Guarded(M * cap, torch.float32, dev, 7.5), Guarded(M * cap, torch.int32, dev, -5), Guarded(M * cap * TOP, torch.int32, dev, -9),
          Guarded(M * cap * TOP, torch.float32, dev, 2.5)]
    state = ops.new_rng_state(3, dev, step=L)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    sp = None if spans is None else torch.tensor(spans, dtype=torch.int32, device=dev)
    rc = _launch(dev, x, torch.from_numpy(tokens).to(dev), ld_tok=cap, state=state, lengths=ln, spans=sp,
                 top_n=torch.tensor([top_n], dtype=torch.int32, device=dev), outs=[o.body for o in gs])
    torch.cuda.synchronize(dev)
    assert rc == 0
    for o in gs:
        assert o.guards_intact()
    got = (gs[0].body.cpu().numpy().reshape(M, cap), gs[1].body.cpu().numpy().reshape(M, cap),
           gs[2].body.cpu().numpy().reshape(M, cap, TOP), gs[3].body.cpu().numpy().reshape(M, cap, TOP))
    outputs = (np.full((M, cap), 7.5, np.float32), np.full((M, cap), -5, np.int32), np.full((M, cap, TOP), -9, np.int32),
               np.full((M, cap, TOP), 2.5, np.float32))
    want = LM.token_logprobs(full, V, tokens, top_n=top_n, L=L, lengths=lengths, spans=spans, outputs=outputs)
    return got, want


def test_finished_and_forced_rows_are_left_alone(dev):
    """L = 6: row 0 running, row 1 finished at 4 (skipped), row 2 stopped AT this position (lengths = L + 1: scored), row 3 forced
    (prompt of 9), row 4 at the first position after its prompt (scored), row 5 finished exactly at L (skipped)"""
    L = 6
    lengths = [0, 4, L + 1, 0, 0, L]
    spans = [[1, 30], [1, 30], [2, 30], [9, 30], [L, 30], [1, 30]]
    got, want = _decode_case(dev, L, 12, lengths, spans)
    assert not LM.compare(got, want)
    for skipped in (1, 3, 5):
        assert (got[0][skipped] == 7.5).all() and (got[1][skipped] == -5).all() and (got[2][skipped] == -9).all()
    for scored in (0, 2, 4):
        assert got[0][scored, L] != 7.5 and got[1][scored, L] != -5 and (got[2][scored, L, 3:] == -1).all()
        assert (np.delete(got[0][scored], L) == 7.5).all()                  # and no other column of a scored row
    # the comparison would catch a kernel that left the stop token unscored
    bad = LM.token_logprobs(*_same_inputs(L, 12, len(lengths)), top_n=3, L=L, lengths=lengths, spans=spans,
                            outputs=tuple(a.copy() for a in _sentinels(len(lengths), 12)), defect="stop_unscored")
    assert LM.compare(got, bad)


def _same_inputs(L, cap, M, V=65, seed=21):
    full, _ = LM.make_case(V, M, "randn1", seed)
    tokens = np.random.default_rng(seed).integers(0, V, size=(M, cap)).astype(np.int64)
    return full, V, tokens


def _sentinels(M, cap):
    return (np.full((M, cap), 7.5, np.float32), np.full((M, cap), -5, np.int32), np.full((M, cap, TOP), -9, np.int32),
            np.full((M, cap, TOP), 2.5, np.float32))


def test_lengths_and_spans_are_each_optional(dev):
    for lengths, spans in (([0, 3, 0], None), (None, [[1, 9], [7, 9], [5, 9]]), (None, None)):
        got, want = _decode_case(dev, 5, 8, lengths, spans, M=3)
        assert not LM.compare(got, want)
        assert got[0][0, 5] != 7.5 and (got[0][1, 5] == 7.5) == (lengths is not None or spans is not None)


def test_position_beyond_the_row_writes_nothing(dev):
    for L in (8, 9, 1 << 20):
        got, want = _decode_case(dev, L, 8, [0, 0], [[1, 30], [1, 30]])
        assert (got[0] == 7.5).all() and (got[1] == -5).all() and (got[2] == -9).all() and (got[3] == 2.5).all()
        assert not LM.compare(got, want)


def test_refusals(dev):
    """every refusal returns non-zero, and launches nothing: the outputs keep their pattern"""
    M, V = 2, 65
    x = torch.zeros((M, V), device=dev)
    tok = torch.zeros(M, dtype=torch.int64, device=dev)
    tok2 = torch.zeros((M, 4), dtype=torch.int64, device=dev)
    from drakegpt_amd import _lib, ops
    state = ops.new_rng_state(0, dev, step=1)
    ln = torch.zeros(M, dtype=torch.int32, device=dev)
    sp = torch.zeros((M, 2), dtype=torch.int32, device=dev)
    lp = Guarded(M * 4, torch.float32, dev)
    ti = Guarded(M * 4 * TOP, torch.int32, dev)
    tl = Guarded(M * 4 * TOP, torch.float32, dev)
    o = (lp.body, None, None, None)
    p, s = ops._p, ops._stream()
    f = _lib.lib.dg_token_logprobs
    assert f(None, 0, V, M, V, p(tok), 0, None, None, None, None, p(lp.body), None, None, None, s) != 0          # NULL logits
    assert f(p(x), 0, V, M, V, None, 0, None, None, None, None, p(lp.body), None, None, None, s) != 0            # NULL tokens
    assert _launch(dev, x, tok2, ld_tok=4, state=None, outs=o) != 0                                              # ld_tok > 0 without state
    assert _launch(dev, x, tok, lengths=ln, outs=o) != 0                                                         # lengths with ld_tok == 0
    assert _launch(dev, x, tok, spans=sp, outs=o) != 0                                                           # spans with ld_tok == 0
    assert _launch(dev, x, tok, outs=(lp.body, None, ti.body, None)) != 0                                        # top_ids without top_lp
    assert _launch(dev, x, tok, outs=(lp.body, None, None, tl.body)) != 0                                        # and the reverse
    for bad_dtype in (_lib.DG_FP8_E4M3, _lib.DG_F32X3, 99, -1):
        assert f(p(x), bad_dtype, V, M, V, p(tok), 0, None, None, None, None, p(lp.body), None, None, None, s) != 0
    assert f(p(x), 0, (1 << 20) + 1, 1, (1 << 20) + 1, p(tok), 0, None, None, None, None, p(lp.body), None, None, None, s) != 0      # V > 2^20
    assert f(p(x), 0, V - 1, M, V, p(tok), 0, None, None, None, None, p(lp.body), None, None, None, s) != 0      # ldl < V
    torch.cuda.synchronize(dev)
    for g in (lp, ti, tl):
        assert g.buf.cpu().numpy().tobytes() == g.before.tobytes()


def test_two_launches_are_bit_identical(dev):
    for V, bf16 in ((4099, False), (50257, True)):
        full, tok = LM.make_case(V, 2, "randn30", 4, bf16)
        a = _run_flat(dev, full, V, tok, bf16, 20)
        b = _run_flat(dev, full, V, tok, bf16, 20)
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()


def test_ops_wrapper_and_functional(dev):
    """ops.token_logprobs / functional.token_logprobs return what the raw entry writes"""
    from drakegpt_amd import functional as HF
    from drakegpt_amd import ops
    full, tok = LM.make_case(80, 8, "quant4", 31)
    want = LM.token_logprobs(full, 80, tok, top_n=5)
    x, t = _device_logits(full, 80, False, dev), torch.from_numpy(tok).clamp(0, 79).to(dev)
    lp = ops.token_logprobs(x, t)
    assert not LM.compare((lp.cpu().numpy(), None, None, None), want)
    lp, rk, ti, tl = ops.token_logprobs(x, t, top_n=5, rank=True)
    assert tuple(ti.shape) == (8, 5)
    assert not LM.compare((lp.cpu().numpy(), rk.cpu().numpy(), None, None), want)
    assert np.array_equal(ti.cpu().numpy(), want[2][:, :5]) and LM.lp_mismatch(tl.cpu().numpy(), want[3][:, :5]) is None
    lp2, rk2 = HF.token_logprobs(x.contiguous().view(2, 4, 80), t.view(2, 4), rank=True)
    assert tuple(lp2.shape) == (2, 4) and torch.equal(lp2.view(-1), lp) and torch.equal(rk2.view(-1), rk)
    with pytest.raises(ValueError):
        ops.token_logprobs(x, t, top_n=21)
