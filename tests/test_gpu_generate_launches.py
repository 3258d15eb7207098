"""The launch trace of generate(), pinned: every library call (the `what` of ops.check) a generate() call makes, in order, the
tokens it returns and, where a DeviceDecoder is involved, which of its graph pairs exist afterwards -- against
tests/golden/generate_launches.json.  The models are driven through the public generate(...) signature only, so the recorder
below runs on any commit that has the device sampler and the controls:

    python tests/test_gpu_generate_launches.py          rewrites tests/golden/generate_launches.json

The golden file was recorded before generate() was restructured (one request, one layer stack, each loop once) and is what that
restructuring is held to; it is not to be re-recorded for a change that is meant to leave generate() as it is.

Model: the tiny TransformerLM of the sampler tests (V 80, C 64, ctx 32, 4 heads, 2 layers, seed 42, eval, fp32) and a BlocksLM of
the same shape for _LM.generate; prompt of 2 tokens, 40 new ones, so every cached case crosses the window at 32."""
import contextlib
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE = os.path.join(ROOT, "tests", "golden", "generate_launches.json")
V, CTX, T0, NEW = 80, 32, 2, 40
NINF = float("-inf")
HOST_CASES = ("host_blocks", "host_blocks_temperature_top_k", "host_cached", "host_uncached", "host_prompt_fills_window", "host_top_p",
              "host_penalty_bias", "host_stop", "host_train")
DEVICE_CASES = ("device_blocks", "device_uncached", "device_train", "device_cached_first", "device_cached_second",
                "device_cached_first_penalty", "device_cached_stop_poll_7", "device_no_new_tokens")
CASES = HOST_CASES + DEVICE_CASES


@contextlib.contextmanager
def _recording(calls):
    from drakegpt_amd import ops
    check = ops.check

    def counting(rc, what):
        calls.append(what)
        return check(rc, what)

    ops.check = counting
    try:
        yield
    finally:
        ops.check = check


def _model(dev, cls="TransformerLM"):
    import drakegpt_amd as D
    torch.manual_seed(42)
    if cls == "BlocksLM":
        return D.BlocksLM(V, 64, CTX, 4, 2).to(dev).eval()
    return D.TransformerLM(V, 64, CTX, 4, 2, 0.0).to(dev).eval()


def _prompt(dev, t0=T0):
    return (torch.arange(t0, dtype=torch.long, device=dev) * 7 + 2).remainder(V)[None].contiguous()


def _run(m, idx, n_new, host, **kw):
    """one traced generate() call -> {"launches", "tokens"} (+ "graphs" when the model has a decoder afterwards)"""
    calls = []
    args = (torch.Generator().manual_seed(0),) if host else ()
    if not host:
        kw = dict(kw, sampler="device", seed=11)
    with _recording(calls):
        out = m.generate(idx, n_new, *args, **kw)
    torch.cuda.synchronize(idx.device)
    res = {"launches": calls, "tokens": out.tolist()}
    decs = list(getattr(m, "_decoders", {}).values())
    if decs:
        assert len(decs) == 1
        res["graphs"] = {"graphs": decs[0].graphs is not None, "graphs_control": decs[0].graphs_control is not None}
    return res


def record_all(dev):
    """every case, in the order of CASES (the cached device cases share one model, in that order)"""
    idx = _prompt(dev)
    res = {}
    res["host_blocks"] = _run(_model(dev, "BlocksLM"), idx, NEW, True)
    res["host_blocks_temperature_top_k"] = _run(_model(dev, "BlocksLM"), idx, NEW, True, temperature=0.8, top_k=10)
    res["host_cached"] = _run(_model(dev), idx, NEW, True, use_cache=True)
    res["host_uncached"] = _run(_model(dev), idx, NEW, True, use_cache=False)
    res["host_prompt_fills_window"] = _run(_model(dev), _prompt(dev, CTX), NEW, True)
    res["host_top_p"] = _run(_model(dev), idx, NEW, True, top_p=0.9)
    res["host_penalty_bias"] = _run(_model(dev), idx, NEW, True, repetition_penalty=1.3, logit_bias={11: NINF})
    stop = res["host_cached"]["tokens"][0][T0 + 19]                   # the plain run's 20th new token
    res["host_stop"] = _run(_model(dev), idx, NEW, True, stop_tokens=stop)
    res["host_train"] = _run(_model(dev).train(), idx, NEW, True)

    res["device_blocks"] = _run(_model(dev, "BlocksLM"), idx, NEW, False)
    res["device_uncached"] = _run(_model(dev), idx, NEW, False, use_cache=False)
    res["device_train"] = _run(_model(dev).train(), idx, NEW, False)
    m = _model(dev)
    res["device_cached_first"] = _run(m, idx, NEW, False)             # prefill, both warm-ups, both captures
    res["device_cached_second"] = _run(m, idx, NEW, False)            # no capture
    res["device_cached_first_penalty"] = _run(m, idx, NEW, False, repetition_penalty=1.3)         # the second pair is captured
    stop = res["device_cached_first"]["tokens"][0][T0 + 19]
    res["device_cached_stop_poll_7"] = _run(m, idx, NEW, False, stop_tokens=stop, stop_poll=7)
    res["device_no_new_tokens"] = _run(_model(dev), idx, 0, False)
    assert tuple(res) == CASES
    return res


@pytest.fixture(scope="module")
def expected():
    with open(FILE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def recorded(dev):
    return record_all(dev)


def test_every_case_is_pinned(expected):
    assert sorted(expected) == sorted(CASES)


def test_the_cases_reach_what_they_are_for(expected):
    """stated on the golden file alone: the paths the cases were chosen for are in it"""
    e = expected
    assert "dg_softmax_rows" in e["host_cached"]["launches"] and "dg_attn_decode" in e["host_cached"]["launches"]
    assert "dg_attn_decode" not in e["host_uncached"]["launches"] + e["host_prompt_fills_window"]["launches"] + e["host_train"]["launches"]
    assert "dg_sample_rows" in e["host_blocks_temperature_top_k"]["launches"]
    assert "dg_sample_rows_nucleus" in e["host_top_p"]["launches"]
    assert "dg_sample_rows_control" in e["host_penalty_bias"]["launches"]
    for stopped, plain in (("host_stop", "host_cached"), ("device_cached_stop_poll_7", "device_cached_first")):
        row = e[stopped]["tokens"][0]                                  # ends at the first occurrence of the plain run's 20th new token
        assert T0 < len(row) <= T0 + 20 and row == e[plain]["tokens"][0][:len(row)] and row[-1] == e[plain]["tokens"][0][T0 + 19]
    assert e["device_cached_first"]["graphs"] == {"graphs": True, "graphs_control": False}
    assert e["device_cached_first_penalty"]["graphs"] == e["device_cached_stop_poll_7"]["graphs"] == {"graphs": True, "graphs_control": True}
    assert len(e["device_cached_second"]["launches"]) < len(e["device_cached_first"]["launches"])
    assert e["device_cached_second"]["tokens"] == e["device_cached_first"]["tokens"] == e["device_uncached"]["tokens"]
    assert len(e["device_cached_stop_poll_7"]["tokens"][0]) < T0 + NEW
    assert e["device_no_new_tokens"]["tokens"] == [[2, 9]]
    for c in CASES:
        if c not in ("host_stop", "device_cached_stop_poll_7", "device_no_new_tokens"):
            assert len(e[c]["tokens"][0]) == (CTX if c == "host_prompt_fills_window" else T0) + NEW, c


@pytest.mark.parametrize("case", CASES)
def test_generate_makes_the_pinned_launches(recorded, expected, case):
    got, want = recorded[case], expected[case]
    assert len(want["launches"]) > 0 or case == "device_no_new_tokens"
    first = next((i for i, (a, b) in enumerate(zip(got["launches"], want["launches"])) if a != b),
                 min(len(got["launches"]), len(want["launches"])))
    assert got["launches"] == want["launches"], (case, "first difference at call", first, got["launches"][first:first + 4],
                                                 want["launches"][first:first + 4])
    assert got["tokens"] == want["tokens"], (case, got["tokens"], want["tokens"])
    assert got.get("graphs") == want.get("graphs"), (case, got.get("graphs"), want.get("graphs"))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    res = record_all(torch.device("cuda:0"))
    with open(sys.argv[1] if len(sys.argv) > 1 else FILE, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in res.items():
        print(k, len(v["launches"]), "calls,", len(v["tokens"][0]), "tokens,", v.get("graphs"))
