"""The launch trace of one optimizer step, pinned: every library call (the `what` of ops.check) and every gradient exchange
(`all_reduce[numel]`) an eager TrainEngine step makes, in order, against tests/golden/step_launches.json -- and, captured, the
number of graphs the step is held in.  The engine is driven through its public calls only (set_batch / stage_offsets, then
step / micro_step), so the recorder below runs on any commit:

    python tests/test_gpu_step_launches.py          rewrites tests/golden/step_launches.json

The configurations are the smallest that reach each path of the step driver: the tiny fp32 model (default, clipping, two
micro-steps of accumulation), tiny bf16 with schedule + decay groups + moving average, and the scaled preset at B 16 (gather
launch, block chain, grouped dW) as a single process, on the multi-rank path with one and with three exchange groups under a
one-rank process group, and in fp8, whose first step seeds the amax histories and whose second does not."""
import contextlib
import json
import os
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILE = os.path.join(GOLDEN, "step_launches.json")
V = 80
CASES = ("tiny_fp32", "tiny_fp32_clip", "tiny_fp32_accum2", "tiny_bf16_schedule_no_decay_ema", "scaled_bf16", "scaled_bf16_dp_1_bucket",
         "scaled_bf16_dp_3_buckets", "scaled_fp8_two_steps")


@contextlib.contextmanager
def _recording(calls):
    import torch.distributed as dist
    from drakegpt_amd import ops
    check, all_reduce = ops.check, dist.all_reduce

    def counting(rc, what):
        calls.append(what)
        return check(rc, what)

    def marking(tensor, *a, **kw):
        calls.append(f"all_reduce[{tensor.numel()}]")
        return all_reduce(tensor, *a, **kw)

    ops.check, dist.all_reduce = counting, marking
    try:
        yield
    finally:
        ops.check, dist.all_reduce = check, all_reduce


@contextlib.contextmanager
def _one_rank_group():
    import torch.distributed as dist
    with tempfile.TemporaryDirectory() as d:
        dist.init_process_group("gloo", init_method="file://" + os.path.join(d, "store"), rank=0, world_size=1)
        try:
            yield dist.group.WORLD
        finally:
            dist.destroy_process_group()


def _tiny(dev, precision, graph, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.engine import TrainEngine
    fix = torch.load(os.path.join(GOLDEN, "traj5_TransformerLM.pt"), weights_only=True)
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.0, precision=precision)
    m.load_state_dict(fix["init"])
    eng = TrainEngine(m.to(dev), 16, 8, lr=1e-3, betas=(0.9, 0.95), use_graph=graph, **kw)
    micro = kw.get("accum_steps", 1)

    def run():
        for j in range(micro):
            eng.set_batch(fix["x"][j][:16].to(dev), fix["y"][j][:16].to(dev))
            eng.micro_step()
    return eng, run


def _scaled(dev, precision, graph, steps=1, dp=False, **kw):
    import drakegpt_amd as D
    from drakegpt_amd.config import PRESETS
    from drakegpt_amd.engine import TrainEngine
    cfg = PRESETS["scaled"]
    T = cfg["context_length"]
    torch.manual_seed(42)
    m = D.TransformerLM(V, cfg["embedding_dim"], T, cfg["num_heads"], cfg["num_layers"], cfg["dropout"], precision=precision).to(dev)
    eng = TrainEngine(m, 16, T, lr=cfg["base_lr"], betas=cfg["betas"], seed=7, use_graph=graph, **kw)
    eng.force_dp_path = dp
    eng.set_corpus(torch.randint(0, V, (20_000,), generator=torch.Generator().manual_seed(1)))
    eng.stage_offsets(torch.randint(20_000 - T - 1, (4, 16), generator=torch.Generator().manual_seed(2)))

    def run():
        for _ in range(steps):
            eng.step()
    return eng, run


def _cases(dev, pg):
    """name -> make(graph) -> (engine, run): run() is one optimizer step (the fp8 case: two)"""
    return {
        "tiny_fp32": lambda g: _tiny(dev, "fp32", g),
        "tiny_fp32_clip": lambda g: _tiny(dev, "fp32", g, max_grad_norm=1.0),
        "tiny_fp32_accum2": lambda g: _tiny(dev, "fp32", g, accum_steps=2),
        "tiny_bf16_schedule_no_decay_ema": lambda g: _tiny(dev, "bf16", g, lr_schedule=[1e-3, 5e-4, 2e-4], no_decay=("bias", "layernorm"),
                                                            ema_decay=0.99),
        "scaled_bf16": lambda g: _scaled(dev, "bf16", g),
        "scaled_bf16_dp_1_bucket": lambda g: _scaled(dev, "bf16", g, dp=True, process_group=pg, dp_buckets=1),
        "scaled_bf16_dp_3_buckets": lambda g: _scaled(dev, "bf16", g, dp=True, process_group=pg, dp_buckets=3),
        "scaled_fp8_two_steps": lambda g: _scaled(dev, "fp8", g, steps=2),
    }


def record_case(dev, pg, name):
    """{"launches": [what, ...] of the eager step, "graphs": len(eng._graphs) after the captured one}"""
    make = _cases(dev, pg)[name]
    calls = []
    eng, run = make(False)
    with _recording(calls):
        run()
    torch.cuda.synchronize(dev)
    eng.check_status()
    eng, run = make(True)
    run()
    torch.cuda.synchronize(dev)
    eng.check_status()
    return {"launches": calls, "graphs": len(eng._graphs)}


@pytest.fixture(scope="module")
def group():
    with _one_rank_group() as pg:
        yield pg


@pytest.fixture(scope="module")
def expected():
    with open(FILE) as f:
        return json.load(f)


def test_every_case_is_pinned(expected):
    assert sorted(expected) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_step_makes_the_pinned_launches(dev, group, expected, case):
    got, want = record_case(dev, group, case), expected[case]
    assert len(want["launches"]) > 0
    first = next((i for i, (a, b) in enumerate(zip(got["launches"], want["launches"])) if a != b),
                 min(len(got["launches"]), len(want["launches"])))
    assert got["launches"] == want["launches"], (case, "first difference at call", first, got["launches"][first:first + 4],
                                                 want["launches"][first:first + 4])
    assert got["graphs"] == want["graphs"], (case, got["graphs"], want["graphs"])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    with _one_rank_group() as pg:
        res = {name: record_case(torch.device("cuda:0"), pg, name) for name in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else FILE, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for k, v in res.items():
        print(k, len(v["launches"]), "calls,", v["graphs"], "graph(s)")
