"""CPU: host-side surface of precision "bf16x3" (fp32 storage, split-bf16 contractions) -- the model switch, the training
harness flag and the C ABI that carries the split operand code."""
import ctypes as C

import pytest
import torch

import drakegpt_amd as D
from drakegpt_amd import _lib, train

V = 80


def test_transformer_constructs_in_bf16x3():
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.1, precision="bf16x3")
    assert m.precision == "bf16x3" and m.act_dtype == torch.float32
    assert m.split_bf16 and m.run_mode == "bf16x3"
    # every sub-module carries the mode (the autograd shells read it per call)
    for sub in m.modules():
        if isinstance(sub, D.model_component.HipModule):
            assert sub.split_bf16 and sub.act_dtype == torch.float32


def test_set_precision_switches_to_and_from_bf16x3():
    m = D.TransformerLM(V, 32, 8, 4, 3, 0.1)
    assert not m.split_bf16 and m.run_mode == torch.float32
    m.set_precision("bf16x3")
    assert all(s.precision == "bf16x3" for s in m.modules() if isinstance(s, D.model_component.HipModule))
    assert m.run_mode == "bf16x3" and m.act_dtype == torch.float32
    m.set_precision("fp32")
    assert not m.split_bf16 and m.run_mode == torch.float32
    with pytest.raises(ValueError):
        m.set_precision("bf16x2")


def test_functional_run_carries_the_split_flag():
    from drakegpt_amd import functional as HF
    r = HF._run("bf16x3", None)
    assert r.split and r.act == torch.float32 and not r.fp8
    for act in (torch.float32, torch.bfloat16, "fp8"):
        assert not HF._run(act, None).split


def test_train_parser_accepts_bf16x3():
    args = train.build_parser().parse_args(["--precision", "bf16x3"])
    assert args.precision == "bf16x3"
    assert train.build_parser().parse_args([]).precision == "bf16"      # the default is unchanged


def test_library_reports_abi_21():
    assert _lib.ABI_VERSION == 21 and _lib.lib.dg_version() == 21
    assert _lib.DG_F32X3 == 4


def _nt_args(in_dtype, out_dtype, K=384):
    a = _lib.GemmNtArgs()
    # dummy, 16-byte aligned addresses: every call below is rejected by argument checks before anything is launched
    a.A, a.B, a.C = 0x10000, 0x20000, 0x30000
    a.M, a.N, a.K = 256, 256, K
    a.lda, a.ldb, a.ldc = K, K, 256
    a.in_dtype, a.out_dtype = in_dtype, out_dtype
    return a


def test_split_code_is_rejected_where_it_is_not_offered():
    lib = _lib.lib
    # dg_gemm_nt: fp32 output only
    a = _nt_args(_lib.DG_F32X3, _lib.DG_BF16)
    assert lib.dg_gemm_nt(C.byref(a), None) == -3
    # no sign-bit / column-sum forms for split operands
    assert lib.dg_gemm_nt_sign_bits_supported(C.byref(_nt_args(_lib.DG_F32X3, _lib.DG_F32))) == 0
    assert lib.dg_gemm_nt_colsum_supported(C.byref(_nt_args(_lib.DG_F32X3, _lib.DG_F32))) == 0
    # the grouped dW GEMM has no split form
    prob = (_lib.TnProblem * 1)()
    assert lib.dg_gemm_tn_grouped(prob, 1, _lib.DG_F32X3, None, 0, None) == -3
