"""CPU: the gradient-clipping entry points are exported and bound, the harness flag parses, and bad thresholds are refused before
anything reaches the GPU."""
import math

import pytest
import torch


def test_library_exports_the_clipping_entry_points():
    from drakegpt_amd import _lib
    for name in ("dg_sumsq_parts", "dg_sumsq_partials", "dg_grad_norm_finalize", "dg_adamw_step_clip"):
        assert hasattr(_lib.lib, name) and name in _lib.SIGNATURES, name
    # the partition depends on n alone: one partial per workgroup, at most 2048
    parts = [int(_lib.lib.dg_sumsq_parts(n)) for n in (1, 5, 1024, 262_147, 10_800_000, 100_000_000)]
    assert parts == [1, 1, 1, 65, 2048, 2048]
    assert _lib.lib.dg_sumsq_parts(0) == 0


def test_clipping_entry_points_reject_bad_arguments():
    from drakegpt_amd import _lib
    lib = _lib.lib
    # null pointers, empty sizes and misaligned buffers are refused before any launch
    assert lib.dg_sumsq_partials(None, 16, 0x10000, None) == -1
    assert lib.dg_sumsq_partials(0x10000, 0, 0x20000, None) == -1
    assert lib.dg_sumsq_partials(0x10004, 16, 0x20000, None) != 0
    assert lib.dg_grad_norm_finalize(0x10000, 0, 1.0, 0x20000, 0x30000, None) == -1
    assert lib.dg_grad_norm_finalize(0x10000, 4, 1.0, None, 0x30000, None) == -1
    assert lib.dg_adamw_step_clip(0x10000, 0x20000, 0x30000, 0x40000, 16, 0x50000, 0x60000, 1.0, None, None, 1, None) == -1


def test_train_parser_grad_clip_flag():
    from drakegpt_amd import train
    assert train.build_parser().parse_args([]).grad_clip is None                  # off by default
    assert train.build_parser().parse_args(["--grad-clip", "1.0"]).grad_clip == 1.0


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "x"])
def test_adamw_rejects_bad_max_grad_norm(bad):
    from drakegpt_amd.optim import AdamW
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(ValueError):
        AdamW([p], max_grad_norm=bad)


def test_adamw_clipping_settings():
    from drakegpt_amd.optim import AdamW, check_max_grad_norm
    p = torch.nn.Parameter(torch.zeros(4))
    assert AdamW([p]).max_grad_norm is None and AdamW([p]).last_grad_norm is None
    opt = AdamW([p], max_grad_norm=2)
    assert opt.max_grad_norm == 2.0 and opt.last_grad_norm is None      # a device scalar once a step has run
    assert check_max_grad_norm(1e-3) == 1e-3 and math.isfinite(check_max_grad_norm(1e30))
