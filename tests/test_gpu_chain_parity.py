"""dg_block_chain_fwd / dg_block_chain_bwd stage by stage against fp64 on the launch's own stored tensors.

The launch tests of tests/test_gpu_ops.py compare the chain with the project's own GEMM and LayerNorm launches by a whole-tensor
ratio; here every intermediate the launch stores (x1, mean2 / rstd2, h2, f, the sign bits, x2, mean1 / rstd1, h1, qkv) is checked
element by element against fp64 evaluated on the stored INPUT of that stage, inside the derived envelopes of oracle/parity.py (the
checks themselves: tests/chain_model.py, shown on the CPU to refuse planted defects by tests/test_parity_host.py).  Shapes follow
the device's CU count, the attribute the kernel sizes its grid by: one block; a grid below one XCD group; CUs + 1 blocks (one
workgroup runs two rounds); 2 CUs + 3 blocks (three workgroups run three rounds, all others two).  C = 384 is the only width.

The separate launches (gemm_nt, layernorm_fwd) are never run on a test's operands in front of the chain: a store the chain skipped
could find the right values in recycled allocator memory.

Measured envelope use (largest error / bound per stage over all cases below, MI355X, 256 CUs, DG_TEST_REPORT=1; recorded, not
asserted -- the assertion is use <= 1 against the derived bound; also in DESIGN.md section 2):

    forward   x1, x2 (fp32)      <= 0.01      K 2^-24 sum |a||b| is the worst case over all summation orders
              mean2 / mean1      0.06 .. 0.16
              rstd2 / rstd1      0.09 .. 0.19
              h2 / h1 (bf16)     0.98 .. 1.00  a bf16 store alone uses up to 1: round-to-nearest moves a value just above a power of
              f (bf16)           0.95 .. 0.98  two by 2^-8 of itself; the fp32 error in front of it is what the envelope is for
              x2 (bf16, mode 1)  0.90 .. 0.97
              qkv (bf16)         0.95 .. 0.98
              sign bits          equal to (stored f > 0) everywhere and to the fp64 sign wherever decided; 1.8e-4 .. 2.5e-4 undecided
    backward  dx1 / g1 (rows)    0.28 .. 0.32  dx2 / g2 (rows)  0.32 .. 0.36
              df                 0.95 .. 0.98  dout             0.95 .. 0.97
              dgamma partials    <= 0.17       dbeta partials   <= 0.11       bias partials <= 0.05       db1 < 0.005
              hidden dh / dh2    0.72 .. 0.76 of their bf16 roundings undecided by the GEMM envelope (see chain_model.check_bwd)"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_model as CM  # noqa: E402

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
C = CM.C


def _ops():
    from drakegpt_amd import ops
    return ops


def _report(msg):
    if os.environ.get("DG_TEST_REPORT"):
        print("[chain-parity] " + msg, flush=True)


def _blocks(shape, cus):
    return {"1": 1, "5": 5, "cus+1": cus + 1, "2cus+3": 2 * cus + 3, "cus": cus}[shape]


def _probe_sign_bits(ops, bits, M, dev):
    """the header declares the layout of the sign bits opaque: read them through their consumer.  ones[M, C] times a [4C, C] matrix
    whose first column is one gives 1 in every element; the masked dX form of dg_gemm_nt returns it where the bit is set."""
    E = torch.zeros(4 * C, C, dtype=bf, device=dev)
    E[:, 0] = 1
    return ops.gemm_nt(torch.ones(M, C, dtype=bf, device=dev), E, torch.float32, K=C, sign_bits=bits)


FWD_CASES = ([(m, s, 0.2) for m in (0, 1, 2) for s in ("1", "5", "cus+1", "2cus+3")]
             + [(m, s, 0.0) for m in (0, 1, 2) for s in ("1", "5")] + [(3, "cus+1", 0.2), (4, "cus+1", 0.2)])


@pytest.mark.parametrize("mode,shape,p", FWD_CASES, ids=[f"mode{m}-{s}-p{p}" for m, s, p in FWD_CASES])
def test_chain_fwd_every_stage_against_fp64_on_its_own_input(dev, mode, shape, p):
    ops = _ops()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    M = CM.ROWS * _blocks(shape, cus)
    assert ops.block_chain_supported(M, C, bf)
    op = CM.fwd_operands(M, M + mode)
    d = {k: v.to(dev) for k, v in op.items()}
    packed = {k: ops.pack_chain_weights(d[k]) for k in CM.WEIGHTS}
    vec = {k: d[k] for k in CM.VECTORS}
    rng = ops.new_rng_state(CM.SEED, dev, CM.STEP) if p > 0 else None
    kw = dict(dropout_p=p, rng_state=rng, site_proj=CM.SITE_PROJ, site_ffn=CM.SITE_FFN, **packed, **vec)
    if mode == 4:
        got = ops.block_chain_fwd(4, M, C, f=d["f_in"], x1=d["x"], **kw)
    else:
        got = ops.block_chain_fwd(mode, M, C, o=d["o"], x=d["x"], **kw)
    mask = _probe_sign_bits(ops, got["bits"], M, dev).cpu() if "bits" in got else None
    torch.cuda.synchronize()
    host = {k: v.cpu() for k, v in got.items() if k != "bits"}
    use = CM.check_fwd(host, op, mode, p, mask=mask, grid=min(cus, M // CM.ROWS))
    _report(f"fwd mode {mode} M={M} ({shape} blocks, {cus} CUs) p={p}: " + " ".join(f"{k} {u:.2e}" if k.startswith("bits") else f"{k} {u:.2f}" for k, u in use.items()))


# dg_block_chain_bwd supports one block per workgroup: a single block, and as many blocks as the device has CUs
BWD_CASES = [(m, s, 0.2) for m in (0, 1, 2) for s in ("1", "cus")] + [(m, "1", 0.0) for m in (0, 1, 2)]


@pytest.mark.parametrize("mode,shape,p", BWD_CASES, ids=[f"mode{m}-{s}-p{p}" for m, s, p in BWD_CASES])
def test_chain_bwd_every_stage_against_fp64_on_its_own_input(dev, mode, shape, p):
    """dx / g of both LayerNorm-backward halves per row, df and dout per element, every column-sum partial per partial row and in
    total: fp64 on the launch's visible tensors (tests/chain_model.py: check_bwd).  The dX GEMM outputs in front of the LayerNorm
    backward exist only in registers, rounded to bf16: the reference rounds its fp64 GEMM of the stored operand the same way."""
    ops = _ops()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    M = CM.ROWS * _blocks(shape, cus)
    assert ops.block_chain_bwd_supported(M, C, bf) and not ops.block_chain_bwd_supported(CM.ROWS * (cus + 1), C, bf)
    op = CM.bwd_operands(M, 7 * M + mode)
    d = {k: v.to(dev) for k, v in op.items()}
    packed = {k: ops.pack_chain_weights(d[k]) for k in CM.BWD_WEIGHTS}
    bits = ops.new_sign_bits(M, 4 * C, dev)
    ops.gemm_nt(d["bits_a"], d["bits_w"], bf, relu=True, sign_bits_out=bits)          # a ReLU pattern from operands of its own
    mask = _probe_sign_bits(ops, bits, M, dev).cpu()
    assert 0.4 < mask.mean().item() < 0.6
    rng = ops.new_rng_state(CM.SEED, dev, CM.STEP) if p > 0 else None
    parts = torch.zeros((2 * (M // CM.ROWS), CM.PART_STRIDE), dtype=torch.float32, device=dev)
    col = lambda name: parts[0, CM.PART_COLS[name][0]:CM.PART_COLS[name][0] + CM.PART_COLS[name][1]]
    has_q, has_2 = mode in (0, 2), mode in (0, 1)
    kw = dict(part_stride=CM.PART_STRIDE, dropout_p=p, rng_state=rng, site_ffn_below=CM.SITE_FFN, site_proj=CM.SITE_PROJ)
    if has_q:
        kw.update(dqkv=d["dqkv"], wqkvT=packed["wqkvT"], x=d["x"], mean1=d["mean1"], rstd1=d["rstd1"], ln1w=d["ln1w"], dresid1=d["dresid"],
                  dln1w_part=col("dln1w"), dln1b_part=col("dln1b"), gbias1_part=col("gbias1") if mode == 0 else None)
    if has_2:
        kw.update(w2T=packed["w2T"], bits=bits, db1_part=col("db1"), w1T=packed["w1T"], x1=d["x1"], mean2=d["mean2"], rstd2=d["rstd2"], ln2w=d["ln2w"],
                  dln2w_part=col("dln2w"), dln2b_part=col("dln2b"), gbias2_part=col("gbias2"), wprojT=packed["wprojT"])
        if mode == 1:
            kw.update(g_in=d["g_in"], dresid2=d["dresid"])
    got = ops.block_chain_bwd(mode, M, C, **kw)
    torch.cuda.synchronize()
    use = CM.check_bwd({k: v.cpu() for k, v in got.items()}, parts.cpu(), op, mode, p, mask)
    _report(f"bwd mode {mode} M={M} ({shape} blocks, {cus} CUs) p={p}: " + " ".join(f"{k} {u:.2f}" for k, u in use.items()))
