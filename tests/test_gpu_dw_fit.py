"""Grouped dW GEMM (dg_gemm_tn_grouped, bf16) at the shapes where its 256 x 128 tiles fit C = 384 badly: tile rows whose
upper half is padding, a single mostly empty tile, ragged edges behind padded leading dimensions, an output view.

Every output element is one dot product over the same K order: it may not depend on whether the upper half of its tile
is padding, on which operand of the MFMA its matrix feeds, or on the launch it ran in.
R = 128 and 192 are two and three K steps (with a workspace: halves of 1 + 1 and 1 + 2 chained through the flags)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 3e-6                      # the bound tests/test_gpu_ops.py sets for gemm_tn_grouped against fp64
# P x Q: C x 4C (2 x 12 tiles, the lower 12 half padding), 4C x C (6 x 3 full tiles), 3C x C (the fifth tile row half padding),
# C x C (second row half padding), V x C (one tile row, mostly padding)
SHAPES = [(384, 1536), (1536, 384), (1152, 384), (384, 384), (80, 384)]


def _ops():
    from drakegpt_amd import ops
    return ops


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def within(got, ref, A, B, K, name):
    """every element within the envelope of an fp32 sum of K exact bf16 products (K = R for a whole tile, R + 1 where two K
    halves are added): a wrong 16-byte chunk or K step that the whole-tensor ratio hides"""
    from oracle import parity
    return parity.assert_within_rounding(got, ref, parity.gemm_envelope(A.T, B.T, K=K), ulps=0, name=name)


def tiles(P, Q):
    """256 x 128 tiles of a P x Q problem"""
    return -(-P // 256) * -(-Q // 128)


_cache = {}


def operands(dev, R, P, Q):
    """random bf16 operands of one problem and the fp64 product, made once per (R, P, Q) and never written"""
    key = (R, P, Q)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * R + 7 * P + Q)
        A = torch.randn(R, P, generator=g).to(torch.bfloat16)
        B = torch.randn(R, Q, generator=g).to(torch.bfloat16)
        _cache[key] = (A.to(dev), B.to(dev), A.double().T @ B.double())
    return _cache[key]


def run(probs, ws):
    ops = _ops()
    for p in probs:
        p[2].fill_(float("nan"))
    ops.gemm_tn_grouped(probs, ws)
    torch.cuda.synchronize()
    return [p[2].clone() for p in probs]


def status(ws):
    return int(ws[-16:].view(torch.int32)[0].item())


@pytest.mark.parametrize("R", [128, 192])
@pytest.mark.parametrize("P,Q", SHAPES)
def test_single_problem(dev, R, P, Q):
    ops = _ops()
    A, B, ref = operands(dev, R, P, Q)
    probs = [(A, B, torch.empty(P * Q, device=dev), P, Q)]
    whole = run(probs, None)[0]
    assert rel(whole.view(P, Q), ref) < TOL, rel(whole.view(P, Q), ref)
    within(whole.view(P, Q), ref, A, B, R, f"{P}x{Q} R={R} whole")
    ws = ops.gemm_tn_grouped_workspace(probs, dev)
    halves = run(probs, ws)[0]                                    # every tile in two K halves, handed over through the workspace
    assert rel(halves.view(P, Q), ref) < TOL, rel(halves.view(P, Q), ref)
    within(halves.view(P, Q), ref, A, B, R + 1, f"{P}x{Q} R={R} halves")
    assert status(ws) == 0


@pytest.mark.parametrize("R", [128, 192])
def test_group_of_all(dev, R):
    """all five in one launch (66 tiles), without and with the workspace; with it twice: bit-equal, flags reset themselves"""
    ops = _ops()
    probs, refs = [], []
    for P, Q in SHAPES:
        A, B, ref = operands(dev, R, P, Q)
        probs.append((A, B, torch.empty(P * Q, device=dev), P, Q))
        refs.append(ref)
    assert sum(tiles(P, Q) for P, Q in SHAPES) == 66
    for o, ref, (P, Q) in zip(run(probs, None), refs, SHAPES):
        assert rel(o.view(P, Q), ref) < TOL, (P, Q, rel(o.view(P, Q), ref))
        within(o.view(P, Q), ref, *operands(dev, R, P, Q)[:2], R, f"group {P}x{Q} R={R} whole")
    ws = ops.gemm_tn_grouped_workspace(probs, dev)
    first, second = run(probs, ws), run(probs, ws)
    for a, b, ref, (P, Q) in zip(first, second, refs, SHAPES):
        assert rel(a.view(P, Q), ref) < TOL, (P, Q, rel(a.view(P, Q), ref))
        within(a.view(P, Q), ref, *operands(dev, R, P, Q)[:2], R + 1, f"group {P}x{Q} R={R} halves")
        assert torch.equal(a, b), (P, Q)
    assert status(ws) == 0


@pytest.mark.parametrize("R", [128, 192])
@pytest.mark.parametrize("P,Q", [(384, 1536), (80, 384), (104, 328)])
def test_exchanged_operands_agree_bitwise(dev, R, P, Q):
    """(A, B) -> P x Q and (B, A) -> Q x P are the same dot products with the operand roles of the MFMA exchanged and other
    tiles (2 x 12 against 6 x 3 at C x 4C): each element must come out bit-identical, whole and in K halves."""
    ops = _ops()
    A, B, _ = operands(dev, R, P, Q)
    probs = [(A, B, torch.empty(P * Q, device=dev), P, Q), (B, A, torch.empty(Q * P, device=dev), Q, P)]
    for ws in (None, ops.gemm_tn_grouped_workspace(probs, dev)):
        o, ot = run(probs, ws)
        assert torch.equal(o.view(P, Q), ot.view(Q, P).T)


@pytest.mark.parametrize("R", [128, 192])
@pytest.mark.parametrize("P,Q", [(100, 1000), (1000, 100), (330, 100), (100, 330)])
def test_padded_operands_and_output_view(dev, R, P, Q):
    """ld > P on both operands (NaN behind the matrix: whatever the clamped loads fetch there must reach no stored element)
    and an output view with ldo > Q (NaN-filled: nothing may be written between the rows).  330 x 100 ends in a ragged tile row
    whose upper half is padding, 1000 x 100 in a ragged full one, 100 x 1000 and 100 x 330 are one ragged, mostly empty row."""
    ops = _ops()
    g = torch.Generator().manual_seed(R + P + Q)
    lda, ldb, ldo = (P + 7) // 8 * 8 + 8, (Q + 7) // 8 * 8 + 16, Q + 5
    A = torch.full((R, lda), float("nan"), dtype=torch.bfloat16)
    A[:, :P] = torch.randn(R, P, generator=g).to(torch.bfloat16)
    B = torch.full((R, ldb), float("nan"), dtype=torch.bfloat16)
    B[:, :Q] = torch.randn(R, Q, generator=g).to(torch.bfloat16)
    ref = A[:, :P].double().T @ B[:, :Q].double()
    Ad, Bd = A.to(dev), B.to(dev)
    out = torch.empty(P, ldo, device=dev)
    probs = [(Ad[:, :P], Bd[:, :Q], out, P, Q)]
    arr, code = ops._tn_problem_array(probs)
    arr[0].ldo = ldo
    ws = ops.gemm_tn_grouped_workspace(probs, dev)
    for w in (None, ws):
        out.fill_(float("nan"))
        ops.check(ops.lib.dg_gemm_tn_grouped(arr, 1, code, w.data_ptr() if w is not None else None,
                                             w.numel() if w is not None else 0, ops._stream()), "dg_gemm_tn_grouped")
        torch.cuda.synchronize()
        assert rel(out[:, :Q], ref) < TOL, rel(out[:, :Q], ref)
        within(out[:, :Q], ref, A[:, :P], B[:, :Q], R + 1, f"padded {P}x{Q} R={R}")
        assert torch.isnan(out[:, Q:]).all()
    assert status(ws) == 0


@pytest.mark.parametrize("R", [128, 192])
def test_half_height_rows_match_full_height(dev, R):
    """640 x 384 tiles as rows of 256 + 256 + 128: the upper half of its last tile row is padding.  The same rows are full tiles
    of the 768 x 384 problem on the same operands, and an element must not depend on what the rest of its tile holds."""
    ops = _ops()
    A, B, ref = operands(dev, R, 768, 384)
    probs = [(A[:, :640], B, torch.empty(640 * 384, device=dev), 640, 384), (A, B, torch.empty(768 * 384, device=dev), 768, 384)]
    for ws in (None, ops.gemm_tn_grouped_workspace(probs, dev)):
        part, full = run(probs, ws)
        assert rel(full.view(768, 384), ref) < TOL
        within(full.view(768, 384), ref, A, B, R + 1, f"768x384 R={R}")
        assert torch.equal(part.view(640, 384), full.view(768, 384)[:640])
