"""dg_block_chain_fwd's per-column vectors (biases, gamma, beta) and dg_pack_chain_weights' image.

The forward chain kernel delivers the vectors of an epilogue through LDS: the loader waves copy them, as extra LDS-DMA pieces of
a ring stage, into an activation part that is free at that moment, and every block a workgroup walks re-stages them (FFN2 overwrites
the parts).  What can go wrong there is checked here with the stage checks of tests/chain_model.py (fp64 on the launch's own stored
input of each stage, inside the derived envelopes of oracle/parity.py; nothing is widened for these shapes):

  * modes 0 .. 4 at one block, two blocks and CUs + 1 blocks (one workgroup walks two blocks: the vectors of its second block are
    staged after FFN2 has overwritten the first block's), p = 0.2, and p = 0 at one block;
  * the seven vectors are slices of ONE fp32 buffer at byte offsets = 16, 48 and 112 mod 128 -- 16-byte aligned as the entry point
    requires, not line-aligned, and not each other's neighbours in the order the kernel uses them -- and everything between and
    behind them holds 1e4: a copy that starts at a wrong offset or runs past a vector's end lands far outside every envelope
    (biases are 0.1 N(0, 1), gamma 1 + 0.1 N);
  * a launch with fresh vectors directly behind a launch of the same shape with different ones, on the same stream: the second
    result is checked against the second set.

The packed weight image is checked for exact equality against the layout formula of csrc/chain.hip, evaluated in torch on the CPU,
for the single and the batched entry, source leading dimension > K included, and one K / 32 odd (the form without stage pairs)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
C = CM.C
SENTINEL = 1e4
# the order of the slices inside the buffer: not the order in which the kernel uses them (CM.VECTORS)
BUFFER_ORDER = ("ln1b", "b1", "bproj", "ln2b", "b2", "ln1w", "ln2w")
BYTE_OFFSETS_MOD_128 = (16, 48, 112)


def _ops():
    from drakegpt_amd import ops
    return ops


def _report(msg):
    if os.environ.get("DG_TEST_REPORT"):
        print("[chain-vectors] " + msg, flush=True)


def place_vectors(op, dev):
    """{name: slice of one device buffer}; the buffer is 1e4 wherever no vector lies"""
    at, pos = {}, 0
    for i, name in enumerate(BUFFER_ORDER):
        want = BYTE_OFFSETS_MOD_128[i % 3] // 4                          # in floats, mod 32
        pos += 64                                                         # a sentinel band of at least 256 B in front of every vector
        pos += (want - pos) % 32
        at[name] = pos
        pos += op[name].numel()
    host = torch.full((pos + 64,), SENTINEL, dtype=torch.float32)
    for name, a in at.items():
        host[a:a + op[name].numel()] = op[name]
    buf = host.to(dev)
    vec = {name: buf[a:a + op[name].numel()] for name, a in at.items()}
    for i, name in enumerate(BUFFER_ORDER):
        assert vec[name].data_ptr() % 128 == BYTE_OFFSETS_MOD_128[i % 3], (name, vec[name].data_ptr() % 128)
    return vec


def _probe_sign_bits(ops, bits, M, dev):
    """the sign bits through their consumer (see tests/test_gpu_chain_parity.py)"""
    E = torch.zeros(4 * C, C, dtype=bf, device=dev)
    E[:, 0] = 1
    return ops.gemm_nt(torch.ones(M, C, dtype=bf, device=dev), E, torch.float32, K=C, sign_bits=bits)


def _launch(ops, mode, M, d, packed, vec, p, rng):
    kw = dict(dropout_p=p, rng_state=rng, site_proj=CM.SITE_PROJ, site_ffn=CM.SITE_FFN, **packed, **vec)
    if mode == 4:
        return ops.block_chain_fwd(4, M, C, f=d["f_in"], x1=d["x"], **kw)
    return ops.block_chain_fwd(mode, M, C, o=d["o"], x=d["x"], **kw)


def _check(ops, got, op, mode, p, M, cus, dev):
    mask = _probe_sign_bits(ops, got["bits"], M, dev).cpu() if "bits" in got else None
    torch.cuda.synchronize()
    host = {k: v.cpu() for k, v in got.items() if k != "bits"}
    return CM.check_fwd(host, op, mode, p, mask=mask, grid=min(cus, M // CM.ROWS))


def _blocks(shape, cus):
    return {"1": 1, "2": 2, "cus+1": cus + 1}[shape]


CASES = [(m, s, 0.2) for s in ("1", "2", "cus+1") for m in range(5)] + [(m, "1", 0.0) for m in range(5)]


@pytest.mark.parametrize("mode,shape,p", CASES, ids=[f"mode{m}-{s}-p{p}" for m, s, p in CASES])
def test_vectors_from_unaligned_slices_between_sentinels(dev, mode, shape, p):
    ops = _ops()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    M = CM.ROWS * _blocks(shape, cus)
    op = CM.fwd_operands(M, 3 * M + mode)
    d = {k: op[k].to(dev) for k in ("o", "x", "f_in") + CM.WEIGHTS}
    packed = {k: ops.pack_chain_weights(d[k]) for k in CM.WEIGHTS}
    vec = place_vectors(op, dev)
    rng = ops.new_rng_state(CM.SEED, dev, CM.STEP) if p > 0 else None
    got = _launch(ops, mode, M, d, packed, vec, p, rng)
    use = _check(ops, got, op, mode, p, M, cus, dev)
    _report(f"mode {mode} M={M} ({shape} blocks) p={p}: " + " ".join(f"{k} {u:.2e}" if k.startswith("bits") else f"{k} {u:.2f}" for k, u in use.items()))


@pytest.mark.parametrize("mode", range(5))
def test_fresh_vectors_behind_a_launch_with_different_ones(dev, mode):
    ops = _ops()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    M, p = 2 * CM.ROWS, 0.2
    op = CM.fwd_operands(M, 11 + mode)
    other = CM.fwd_operands(M, 1011 + mode)                              # only its vectors are used
    d = {k: op[k].to(dev) for k in ("o", "x", "f_in") + CM.WEIGHTS}
    packed = {k: ops.pack_chain_weights(d[k]) for k in CM.WEIGHTS}
    vec_other, vec = place_vectors({k: -3.0 * other[k] for k in CM.VECTORS}, dev), place_vectors(op, dev)
    rng = ops.new_rng_state(CM.SEED, dev, CM.STEP)
    _launch(ops, mode, M, d, packed, vec_other, p, rng)
    got = _launch(ops, mode, M, d, packed, vec, p, rng)                  # same stream, nothing in between
    _check(ops, got, op, mode, p, M, cus, dev)


# ---------------------------------------------------------------------------------------------------------------------
# the packed image
# ---------------------------------------------------------------------------------------------------------------------
def packed_image(W):
    """csrc/chain.hip: stage k = (column chunk c = k / (K / 32), K step t = k % (K / 32)); inside a stage 192 lines of 128 B, physical
    16-byte slot s of line j holds logical slot ls = s ^ (j & 7): row c * 384 + j + 192 * (ls >> 2), columns t * 32 + 8 * (ls & 3) .. + 7"""
    N, K = W.shape
    KT = K // 32
    k = torch.arange((N // 384) * KT).view(-1, 1, 1, 1)
    line, slot, e = torch.arange(192).view(1, -1, 1, 1), torch.arange(8).view(1, 1, -1, 1), torch.arange(8).view(1, 1, 1, -1)
    ls = slot ^ (line & 7)
    row = (k // KT) * 384 + line + 192 * (ls >> 2)
    col = (k % KT) * 32 + 8 * (ls & 3) + e
    return W[row, col].reshape(N, K)


def _as_bits(t):
    return t.contiguous().view(torch.int16)


PACK_SHAPES = [(384, 384), (384, 96), (1536, 384), (384, 1536), (1152, 384)]


def _sources(dev, seed):
    """[N, K] bf16 operands, every second one a view with ld > K (16-byte aligned, not line-aligned) inside a sentinel-filled parent"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (N, K) in enumerate(PACK_SHAPES):
        W = torch.randn(N, K, generator=g).to(bf)
        if i % 2:
            parent = torch.full((N, K + 40), SENTINEL, dtype=bf)
            parent[:, 8:8 + K] = W
            Wd = parent.to(dev)[:, 8:8 + K]
            assert Wd.stride(0) == K + 40
        else:
            Wd = W.to(dev)
        out.append((W, Wd))
    return out


def test_packed_image_equals_the_layout_formula(dev):
    ops = _ops()
    for W, Wd in _sources(dev, 5):
        got = ops.pack_chain_weights(Wd).cpu()
        assert torch.equal(_as_bits(got), _as_bits(packed_image(W))), tuple(W.shape)


def test_batched_packed_image_equals_the_layout_formula(dev):
    ops = _ops()
    src = _sources(dev, 6)
    outs = [torch.full(W.shape, SENTINEL, dtype=bf, device=dev) for W, _ in src]
    table, n_desc, total = ops.make_pack_table([(Wd, o) for (_, Wd), o in zip(src, outs)], dev)
    assert total == sum((N // 384) * (K // 32) for N, K in PACK_SHAPES)
    ops.pack_chain_weights_batched(table, n_desc, total)
    torch.cuda.synchronize()
    for (W, _), o in zip(src, outs):
        assert torch.equal(_as_bits(o.cpu()), _as_bits(packed_image(W))), tuple(W.shape)
