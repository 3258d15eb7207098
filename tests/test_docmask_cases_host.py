"""CPU: tests/docmask_cases.py -- the stitched reference is the masked softmax, the case table is what tests/test_gpu_docmask.py
says it is, and the operand draws of the cases are well conditioned for the offset-window bound (read from the reference alone)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_cases as A  # noqa: E402
import docmask_cases as D  # noqa: E402
from oracle import parity as P  # noqa: E402

# (case, draw): attention_cases.dq_conditioning with the offset-window bound at p = 0 / 0.2, measured on the CPU
CONDITIONING = {"doc-one-tile": (0, 0.59, 0.35), "doc-ragged": (1, 0.34, 0.42), "doc-pairs": (0, 0.47, 0.54), "doc-heavy": (3, 0.39, 0.48)}


def test_case_table():
    assert D.NAMES == ["doc-one-tile", "doc-ragged", "doc-pairs", "doc-heavy"]
    assert D.PS == (0.0, 0.2) and len(D.CASE_P) == 8
    want = {"doc-one-tile": (2, 32, (0, 1, 5, 31), 0), "doc-ragged": (3, 66, (0, 31, 33, 64), 0),
            "doc-pairs": (2, 128, (0, 40, 64, 100), 1), "doc-heavy": (1, 512, (0, 130, 256, 300, 511), 2)}
    for c in D.CASES:
        assert (c.B, c.T, c.firsts, c.order) == want[c.name] and c.NH == 3
        assert A.supported(c.B, c.T, c.NH)
        assert A.order(c.B, c.T, c.NH, 256)[0] == c.order                      # (the GPU tests assert it with the device's CU count)
        assert c.draw == CONDITIONING[c.name][0]
    assert set(CONDITIONING) == set(D.NAMES)


def test_starts_follow_the_definition():
    """start[t] = 1 + the last separator before t; the layout helpers agree with a plain loop over the ids"""
    for c in D.CASES:
        ids = D.ids_of(c.T, c.firsts, sep=7, other=3).tolist()
        want = [1 + max([j for j in range(t) if ids[j] == 7], default=-1) for t in range(c.T)]
        s = D.starts_of(c.T, c.firsts)
        assert s.tolist() == want
        assert bool((s <= torch.arange(c.T)).all()) and bool((s[1:] >= s[:-1]).all())
        assert bool(((s[1:] == s[:-1]) | (s[1:] == torch.arange(1, c.T))).all())
        assert D.starts_tensor(c.B, c.T, c.firsts).view(c.B, c.T)[-1].tolist() == want


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_stitched_probabilities_are_the_masked_softmax(p):
    """the stitched P equals a direct fp64 softmax under the mask start[i] <= j <= i to 1e-12; so do Pd, lse and out"""
    B, T, NH, firsts = 2, 40, 2, (0, 1, 9, 32, 39)
    qkv, dout = A.operands(B, T, NH, 5)
    keep = None if p == 0 else torch.from_numpy(A.keep_slab(p, 0, B * NH * T * T).reshape(B, NH, T, T)).double()
    R = D.stitched(qkv, dout, B, T, NH, A.HD, firsts, keep, p)
    q, k, v = P._split(qkv, B, T, NH, A.HD)
    s = (q @ k.transpose(-2, -1) * A.HD ** -0.5).masked_fill(~D.mask(T, firsts), float("-inf"))
    Pm = torch.softmax(s, -1)
    assert (R["P"] - Pm).abs().max().item() < 1e-12
    assert bool((R["P"][:, :, ~D.mask(T, firsts)] == 0).all())
    Pd = Pm if keep is None else Pm * keep / (1 - p)
    assert (R["Pd"] - Pd).abs().max().item() < 1e-12
    assert (R["lse"] - torch.logsumexp(s, -1)).abs().max().item() < 1e-12
    assert (R["out"] - P._pack(Pd @ v)).abs().max().item() < 1e-12
    # the gradients are those of autograd through the masked softmax
    qd = P.f64(qkv).requires_grad_(True)
    q, k, v = qd.view(B, T, 3, NH, A.HD).permute(2, 0, 3, 1, 4)
    w = torch.softmax((q @ k.transpose(-2, -1) * A.HD ** -0.5).masked_fill(~D.mask(T, firsts), float("-inf")), -1)
    w = w if keep is None else w * keep / (1 - p)
    P._pack(w @ v).backward(P.f64(dout))
    got = torch.stack([R["dq"], R["dk"], R["dv"]], 1).reshape(B * T, -1)
    assert (got - qd.grad).abs().max().item() < 1e-11


@pytest.mark.parametrize("name", D.NAMES)
def test_draws_are_well_conditioned_and_every_group_has_a_bound(name):
    """attention_cases.dq_conditioning < 1 for exactly the draws the GPU tests use, from the reference alone; no case and no
    group is left out of the bounds: every (batch, position, head) group has one, and it is at least BWD_MARGIN x the rounding
    model's error of the group itself (a group lies inside its own window)."""
    c = D.case(name)
    draw, c0, c2 = CONDITIONING[name]
    assert c.draw == draw
    for p, want in ((0.0, c0), (0.2, c2)):
        assert (name, p) in D.CASE_P
        R = D.reference(name, p)
        cond = A.dq_conditioning(R, c.B, c.T, c.NH)
        print(f"{name} p={p}: dq_conditioning {cond:.3f} (recorded {want})")
        assert cond < 1.0, cond
        assert abs(cond - want) < 0.02, (cond, want)
        for n in ("dq", "dk", "dv"):
            b = R["bounds"][n]
            assert b.shape == (c.B * c.T * c.NH,) and bool(torch.isfinite(b).all())
            assert bool((b >= P.BWD_MARGIN * R["model_err"][n] * (1 - 1e-12)).all())
        assert R["starts"].dtype == torch.int32 and R["starts"].numel() == c.B * c.T
        assert np.array_equal(R["starts"].view(c.B, c.T)[0].numpy(), D.starts_of(c.T, c.firsts).numpy().astype(np.int32))
