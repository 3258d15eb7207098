"""Graph-captured training step for TransformerLM -- the performance path.

One step = ref: src/train.py:143-151 (get_batch -> forward -> zero_grad -> backward -> AdamW.step)
run as hand-sequenced HIP kernels with no autograd, captured once into a hipGraph and replayed:
Python issues the step's library calls (66 for the scaled preset in bf16, L = 6: tests/golden/step_launches.json) once, at capture
time, and one graph launch per step afterwards.

MI355X-first layout (288 GB HBM: keep everything resident, nothing is re-packed per step):
  * ONE flat fp32 master buffer holds every parameter; the model's nn.Parameters (reference
    state_dict layout, per-head key/query/value) are re-pointed to be VIEWS into it, with each
    layer's heads laid out as one packed [3C, C] QKV operand.  Regions:
        A  GEMM weights      (gradients written by ONE grouped dW launch; fp32 mode: S split-K slabs from the TN GEMMs)
        B  biases, LayerNorm (gradients arrive as G row-chunk partials)
        E  embeddings        (gradients written directly)
        Z  ln_f              (exists for the checkpoint; no gradient, no optimizer update)
  * flat gradient / Adam m / Adam v buffers with the same layout; one fused AdamW launch, which
    also refreshes the bf16 shadow copy of the weights and moves the step counter on; the W^T shadows (dX
    operands, one flat buffer) are refreshed by one batched transpose launch;
  * step counter, dropout seed, learning rate and the staged block of window offsets live in device
    memory, so a replay sees fresh dropout masks, the right bias correction, the scheduler's current lr
    and its own row of offsets (get_batch runs inside the embedding launch);
  * data parallel: the flat gradient is all-reduced (RCCL via torch.distributed) between the
    backward graph and the optimizer graph -- or, bucketed, range by range while the next layer group's
    backward graph runs (_dp_plan); ln_f is outside the reduced range on every rank.

The step is described once, by _step_programs(): the backward programs in order (_prog_fwd_bwd; or _prog_micro, accum_steps
times; or the layer-group segments of _prog_segments), each with the exchange behind it, and the update program _prog_update.
_run() executes that description -- the programs themselves, or their graphs' replay -- for step() and micro_step();
_capture() warms the same programs up and captures them through capture_after_warmup(), which eval_losses and the device
decoder use too.
"""
from __future__ import annotations

import contextlib
import functools
import math
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import checkpoint as CK
from . import ops
from . import schedules as SCH
from . import sublayers as S
from .model import TransformerLM
from .optim import check_accum_steps, check_max_grad_norm

Tensor = torch.Tensor
ALIGN = 64          # floats: every tensor starts on a 256-byte boundary of the flat buffer


def _round(n: int, a: int = ALIGN) -> int:
    return (n + a - 1) // a * a


class _Layout:
    def __init__(self):
        self.entries: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.size = 0

    def add(self, key: str, shape) -> int:
        off = self.size
        self.entries[key] = (off, tuple(shape))
        self.size = off + _round(math.prod(shape))
        return off


WHOLE = "whole"     # the exchange behind a backward program: one synchronous all-reduce of the whole gradient buffer


def capture_after_warmup(dev, progs, restore=None) -> tuple:
    """one hipGraph per program, all in the first one's memory pool (activations may cross from one program to the next).  The
    programs first run once on a side stream -- that loads every code object and makes every allocation a capture could not --
    and restore(), if given, puts back what that run moved before the capture starts."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for prog in progs:
            prog()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize(dev)
    if restore is not None:
        restore()
        torch.cuda.synchronize(dev)
    graphs = []
    for prog in progs:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=graphs[0].pool() if graphs else None):
            prog()
        graphs.append(g)
    return tuple(graphs)


class ShadowWeights:
    """persistent GEMM operands: bf16 (or the fp32 master itself) for forward, W^T for dX"""

    def __init__(self):
        self.fwd_map: Dict[int, Tensor] = {}
        self.bwd_map: Dict[int, Tensor] = {}
        self.fwd8_map: Dict[int, Tuple[Tensor, Tensor]] = {}      # fp8 mode: (e4m3 copy, dequantisation scale [1])
        self.bwd8_map: Dict[int, Tuple[Tensor, Tensor]] = {}
        self.pack_map: Dict[int, Tensor] = {}                      # proj / second FFN Linear in dg_block_chain_fwd's streaming order
        self.packT_map: Dict[int, Tensor] = {}                     # the W^T operands in dg_block_chain_bwd's streaming order
        self.bwd_stale: set = set()                                # precision fp8: matrices whose bf16 W^T is no longer refreshed (only the e4m3 W^T is read)

    def fwd(self, W: Tensor) -> Tensor:
        return self.fwd_map[W.data_ptr()]

    def bwd(self, W: Tensor) -> Tensor:
        if W.data_ptr() in self.bwd_stale:
            raise RuntimeError("drakegpt_amd: the bf16 W^T of this matrix is not maintained in precision fp8 (its e4m3 W^T is)")
        return self.bwd_map[W.data_ptr()]

    def fwd8(self, W: Tensor):
        return self.fwd8_map[W.data_ptr()]

    def pack(self, W: Tensor) -> Optional[Tensor]:
        return self.pack_map.get(W.data_ptr())

    def packT(self, W: Tensor) -> Optional[Tensor]:
        return self.packT_map.get(W.data_ptr())

    def bwd8(self, W: Tensor):
        return self.bwd8_map[W.data_ptr()]


class FlatSink:
    def __init__(self, eng: "TrainEngine"):
        self.e = eng
        self.deferred = []           # (dY, X, dW view, P, Q): operands stay referenced until the grouped launch
        self.small_pending = []      # (slabs, n, splits, out): split-K partials of the small problems, reduced at the next flush

    def defer(self, key, dy, x, P, Q) -> bool:
        if not self.e.grouped_dw:
            return False
        if key in self.e.small_dw:
            return False                              # bucketed data-parallel step, tiny problem: own split-K launch (matrix())
        off, shape = self.e._region(key)              # GEMM weights, or the token table (one-hot dY)
        assert shape == (P, Q), (key, shape, P, Q)
        self.deferred.append((dy, x, self.e.gflat[off:off + P * Q], P, Q))
        return True

    def flush(self, group: int = 0):
        """one grouped launch for everything deferred so far (the whole backward pass, or one layer group of a bucketed
        data-parallel step: every group has its own problem set, hence its own workspace).  precision "fp8": the problems whose
        two operands exist as fp8 copies by now -- every block Linear: the e5m2 dY its dX GEMM consumed, the e4m3 X its forward
        GEMM consumed -- go into a second grouped launch on those copies (dg_gemm_tn_grouped, DG_FP8_E5M2)."""
        if self.deferred:
            bf, f8 = [], []
            for dy, x, view, P, Q in self.deferred:
                d8, x8 = getattr(dy, "dg_fp8", None), getattr(x, "dg_fp8x", None)
                if (self.e.fp8_dw and d8 is not None and x8 is not None and dy.shape[0] % 128 == 0 and d8[0].shape == (dy.shape[0], P)
                        and x8[0].shape == (x.shape[0], Q) and ops._ld(d8[0]) % 16 == 0 and ops._ld(x8[0]) % 16 == 0):
                    f8.append((d8[0], x8[0], view, P, Q, d8[1], x8[1]))
                else:
                    S._refuse_unwritten(dy)
                    S._refuse_unwritten(x)
                    bf.append((dy, x, view, P, Q))
            for kind, probs in ((0, bf), (1, f8)):
                if not probs:
                    continue
                ws = self.e.tn_workspaces.get((group, kind))
                if ws is None:                         # first step: sized for this problem set, zero-filled once
                    ws = self.e.tn_workspaces[(group, kind)] = ops.gemm_tn_grouped_workspace(probs, self.e.dev)
                ops.gemm_tn_grouped(probs, ws)
            self.deferred = []
        for slab, n, splits, out in self.small_pending:
            ops.reduce_partials(slab, n, splits, out, n)
        self.small_pending = []

    def matrix(self, key, P, Q):
        if key in self.e.small_dw:
            # a few-tile problem (lm_head / token table at a char-level vocabulary) inside a bucketed step: as one more problem
            # of a 126-tile group it would push the grouped launch past one round of half tiles, so it gets its own split-K
            # launch into a small slab buffer, summed into the flat gradient right away (deterministic order)
            slab, n = self.e.small_dw[key]
            goff, shape = self.e._region(key)
            assert shape == (P, Q), (key, shape, P, Q)
            self.small_pending.append((slab, P * Q, n, self.e.gflat[goff:goff + P * Q]))
            return slab, P * Q, n
        off, shape = self.e.layA.entries[key]
        assert shape == (P, Q), (key, shape, P, Q)
        # slabs beyond this matrix's own split count are never written: they stay zero from allocation
        n = S.splits_for_matrix(P, Q, self.e.M, self.e.S, self.e.dev)
        return self.e.slabs[0, off:off + P * Q], self.e.layA.size, n

    def vector(self, key, N):
        off, shape = self.e.layB.entries[key]
        assert shape == (N,), (key, shape, N)
        return self.e.vparts[0, off:off + N], self.e.layB.size, self.e.G

    def vector_rows(self, key, N, rows):
        off, shape = self.e.layB.entries[key]
        assert shape == (N,), (key, shape, N)
        if rows > self.e.vparts.shape[0]:
            return None
        # partial rows beyond `rows` are never written for this key: they stay zero from allocation
        return self.e.vparts[:rows, off:off + N]

    def direct(self, key, shape=None):
        return self.e.grad_view(key)


class TrainEngine:
    OFFSET_ROWS = 512          # rows of the staged window-offset block allocated up front (stage_offsets grows it on demand)

    def __init__(self, model: TransformerLM, batch_size: int, context_length: Optional[int] = None, *,
                 lr: float = 1e-3, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 1e-2,
                 seed: int = 42, rank: int = 0, world_size: int = 1, process_group=None, use_graph: bool = True,
                 dp_buckets: Optional[int] = None, logits: str = "auto", grad_stream: str = "auto", fp8_dw: Optional[bool] = None,
                 max_grad_norm: Optional[float] = None, accum_steps: int = 1, lr_schedule=None, schedule_steps: Optional[int] = None,
                 no_decay=(), label_smoothing: float = 0.0, z_loss: float = 0.0, ema_decay: Optional[float] = None,
                 ema_warmup: bool = False, ignore_index: Optional[int] = None, skip_nonfinite: bool = False,
                 skip_grad_norm: Optional[float] = None, doc_separator: Optional[int] = None):
        """doc_separator (a token id; None: off, nothing of it exists): document-masked attention.  A document
        of the packed batch ends WITH this token and no token attends across it, in every program that gathers or embeds a batch
        (step, micro-step, eval_loss, eval_losses; eager and captured): one dg_doc_starts launch behind the embedding launch fills
        an int32 [B*T] buffer on the device and every attention call of the program reads it.
        skip_nonfinite / skip_grad_norm: the update guard (off by default).  The optimizer update of a
        step is applied only if the global gradient norm is at most skip_grad_norm (skip_nonfinite alone: if it is finite) and the
        step's loss is finite; otherwise it is skipped on the device, inside the same captured graph, with no host sync.  A skipped
        step leaves weights, moments, the bf16 shadow, every weight-derived copy, the moving average and the optimizer's step word
        (bias correction, LR-table index, EMA warm-up) untouched, bit for bit, while the data side (dropout key, staged offset
        row, fp8 amax slot, micro-step counter) moves on to the next batch.  The sum of squares is taken in fp32: a gradient
        element beyond 1.8e19 in magnitude reads as non-finite.  With more than one rank the decision rests on the all-reduced
        gradient alone (the same on every rank); a rank's own loss is not consulted.  precision fp8: weights, moments and
        checkpoints stay clean, but an amax history that has itself gone NaN is not healed (its scale stays NaN on purpose)."""
        if not isinstance(model, TransformerLM):
            raise TypeError("TrainEngine drives TransformerLM (the other five models train through the autograd path)")
        p0 = next(model.parameters())
        if not p0.is_cuda:
            raise RuntimeError("TrainEngine needs the model on the GPU (model.to('cuda')); there is no CPU path")
        self.model = model
        self.dev = p0.device
        self.act = model.act_dtype
        self.fp8 = bool(getattr(model, "fp8", False))
        # precision "bf16x3": the fp32 program (act fp32: split-K dW slabs, no chain kernel, no grouped dW) with every GEMM
        # contracted as split bf16
        self.split_bf16 = bool(getattr(model, "split_bf16", False))
        self.fp8_sites: Dict[str, Tensor] = {}
        self._fp8_seeded = False
        self._fp8_keep = False      # load_state_dict: the histories are loaded state, a capture warm-up must put them back
        self._finite_work = None
        self.B = int(batch_size)
        self.T = int(context_length or model.context_length)
        if self.T > model.context_length:
            raise ValueError("context_length exceeds the model's position table")
        self.V, self.C = model.token_embedding_table.weight.shape
        self.L = len(model.blocks)
        blk0 = model.blocks[0]
        self.NH = len(blk0.sa_head.heads)
        self.H = blk0.sa_head.heads[0].head_size
        self.p_drop = float(model._p)
        self.M = self.B * self.T
        self.rank, self.world, self.pg = rank, world_size, process_group
        self.use_graph = use_graph
        self._dp_buckets_arg = dp_buckets
        # gradient accumulation: accum_steps micro-batches per AdamW step (1: nothing below exists, the step is what it always was)
        self.accum = check_accum_steps(accum_steps)
        # (validated before anything is allocated) the learning-rate table of lr_schedule -- a sequence, a 1-D tensor, or a callable
        # s -> lr with schedule_steps entries -- and the kinds of parameter kept out of weight decay
        self.lr_table_host = None if lr_schedule is None else SCH.as_table(lr_schedule, schedule_steps)
        if lr_schedule is None and schedule_steps is not None:
            raise ValueError("schedule_steps goes with lr_schedule")
        self.no_decay = CK.check_no_decay(no_decay)
        # the training objective's options (label smoothing, z-loss: inside the loss-head kernels): what every training program
        # adds to its loss-head call -- nothing for a default engine, whose calls are the ones they always were.  eval_loss /
        # eval_losses stay the plain cross entropy.
        self.label_smoothing, self.z_loss = ops.check_loss_options(label_smoothing, z_loss)
        self._loss_kw = {k: v for k, v in (("label_smoothing", self.label_smoothing), ("z_loss", self.z_loss)) if v != 0.0}
        # ignore_index (F.cross_entropy's; None: off, nothing below exists): a property of the targets, so it holds in every program
        # with a loss head, evaluation included.  token_count = {N, 1 / N} of the batch the last loss head saw, written by one
        # count launch right before it; the head's gradient scale is then 1.0 and the 1 / N comes from the device.
        self.ignore_index = ops.check_loss_options(ignore_index=ignore_index)[2]
        self.token_count = None if self.ignore_index is None else torch.zeros(2, dtype=torch.float32, device=self.dev)
        # the document mask (None: off, nothing below exists): like ignore_index a property of the data, so it holds in every program.
        # doc_starts = the first visible key of every query of the batch in flight, written by one launch behind the embedding
        if doc_separator is not None and (isinstance(doc_separator, bool) or not isinstance(doc_separator, int)
                                          or not 0 <= doc_separator < self.V):
            raise ValueError(f"doc_separator {doc_separator!r} is not a token id in [0, {self.V})")
        self.doc_separator = doc_separator
        self.doc_starts = None if doc_separator is None else torch.zeros(self.M, dtype=torch.int32, device=self.dev)
        # an exponential moving average of the weights, moved on inside the AdamW launch (None: no average, nothing below exists)
        self.ema_decay = ops.check_ema_options(ema_decay, ema_warmup)
        self.ema_warmup = bool(ema_warmup)
        # the update guard (off: nothing of it exists): whether it is on, and the norm limit as given (None: non-finite only)
        self.guard_on, _guard_limit = ops.check_guard_options(skip_nonfinite, skip_grad_norm)
        self.skip_grad_norm = None if skip_grad_norm is None else _guard_limit
        if self.accum > 1 and dp_buckets is not None and int(dp_buckets) > 1:
            raise ValueError("accum_steps > 1 uses one gradient exchange per optimizer step (it is amortised over the micro-steps "
                             "already): dp_buckets > 1 cannot be combined with it")
        env = os.environ.get
        if logits == "auto" and env("DG_LOGITS") in ("fp32", "bf16"):      # A/B runs
            logits = env("DG_LOGITS")
        if grad_stream == "auto" and env("DG_GRAD_STREAM") in ("fp32", "bf16"):
            grad_stream = env("DG_GRAD_STREAM")
        if grad_stream not in ("auto", "fp32", "bf16"):
            raise ValueError("grad_stream must be 'auto', 'fp32' or 'bf16'")
        # The gradient that flows down the residual branch (dresid -> dx of every LayerNorm backward).  bf16 / fp8 modes keep it
        # in bf16 ("auto"): it is rounded once per sub-layer like every other activation gradient of those modes, and every
        # LayerNorm backward moves 75 MB instead of 100 MB.  The forward residual stream stays fp32 in every mode.
        _can = self.act == torch.bfloat16 and ops.layernorm_bwd_fused_supported(self.C) and self.M % 64 == 0
        if grad_stream == "bf16" and not _can:
            raise ValueError("a bf16 gradient stream needs the bf16 / fp8 precision and the fused LayerNorm backward")
        self.stream_dtype = torch.bfloat16 if (_can and grad_stream != "fp32") else torch.float32
        if logits not in ("auto", "fp32", "bf16"):
            raise ValueError("logits must be 'auto', 'fp32' or 'bf16'")
        # logits as bf16 (in-place gradient): by default only where they are big enough to matter -- the GPT-2 vocabulary --
        # and never in the fp32 parity mode; "fp32" keeps what the module path returns (tests compare the two)
        self.bf16_logits = self.act == torch.bfloat16 and 4096 < self.V <= 53248 and logits != "fp32" if logits != "bf16" else True
        if self.bf16_logits and (self.act != torch.bfloat16 or not (4096 < self.V <= 53248)):
            raise ValueError("bf16 logits need the bf16 / fp8 precision and a vocabulary of 4097 .. 53248 (the whole-row kernel)")
        g = S.granule(self.act)
        if self.C % g or (self.NH * self.H) % g:
            raise ValueError(f"embedding_dim must be a multiple of {g} for {self.act}")
        self.S = S.n_splits_for(self.M)
        self.G = S.n_partials_for(self.M)
        # bf16: every dW of the step comes from ONE grouped GEMM at the end of backward, written straight into the
        # flat gradient (no split-K slabs); fp32 parity mode keeps the per-matrix split-K path
        self.grouped_dw = self.act == torch.bfloat16 and self.M % 64 == 0
        self.last_block_act = env("DG_LAST_BLOCK_ACT", "1") != "0"      # 0: fp32 output + cast launch (A/B runs)
        self.fp8_head = False       # (set in _alloc_and_adopt: precision fp8 at a large vocabulary)
        # precision "fp8": the weight gradients of the block Linears on the fp8 copies of their operands (DG_FP8_DW=0: bf16 dW, A/B)
        self.fp8_dw = self.fp8 and (env("DG_FP8_DW", "1") != "0" if fp8_dw is None else bool(fp8_dw))
        # Everything between two attention calls as ONE launch per layer (dg_block_chain_fwd modes 2 / 0 / 1; forward launches per block
        # 7 -> 2): the default where the kernel exists (bf16, C = 384, M % 64 == 0); DG_CHAIN=0 keeps the separate launches (A/B).
        # Same box, headline configuration: 2.507 -> 2.403 ms per step.
        self.chain_full = (env("DG_CHAIN", "1") != "0" and not self.fp8 and self.NH * self.H == self.C and self.last_block_act
                           and ops.block_chain_supported(self.M, self.C, self.act))
        self.chain_warm = env("DG_CHAIN_WARM", "0") == "1"
        # The same for the backward pass (dg_block_chain_bwd: dX-QKV + LayerNorm-1 backward of block l, dX-FFN2 / dX-FFN1 / LayerNorm-2
        # backward / dX-proj of block l - 1 in one launch; backward launches per block 8 -> 3).  Needs the bf16 gradient stream and one
        # gradient exchange (a chain straddles two blocks: no layer-group seams).  Opt-in (DG_CHAIN_BWD=1) until it beats the separate launches
        # inside the step (first measurement: 136 vs 128.5 us per layer).
        self.chain_bwd = (env("DG_CHAIN_BWD", "0") == "1" and self.chain_full and self.stream_dtype == torch.bfloat16
                          and ops.block_chain_bwd_supported(self.M, self.C, self.act))
        # LayerNorm inside the epilogue of the GEMM that produces its input (dg_block_chain_fwd modes 3 / 4: proj + residual + LN2,
        # FFN2 + residual + the next block's LN1): bf16 mode at the width the kernel is built for.  OFF by default (DG_CHAIN_LN=1 turns
        # it on): measured inside the captured step (round 3, same box) proj + LN2 24.7 us against 17.4 + 8.8, FFN2 + LN1' 44.2 us
        # against 33.5 + 8.8, plus 7.8 us for the packed-weight refresh: 2.558 vs 2.528 ms per step
        self.chain_ln = (env("DG_CHAIN_LN", "0") == "1" and not self.fp8 and self.NH * self.H == self.C
                         and ops.block_chain_supported(self.M, self.C, self.act))
        self._build_layout()
        self.dp_buckets = self._choose_buckets(self._dp_buckets_arg)
        if self.dp_buckets > 1:
            self.chain_bwd = False
        self._alloc_and_adopt()
        if self.fp8_head and self.z_loss > 0.0:
            # the loss kernel's e5m2 gradient copy is scaled a priori by 57344 M: |dlogits| <= 1 / M, which label smoothing
            # keeps and a z-loss does not (a gradient row sums to 2 z_loss lse / M)
            raise ValueError("z_loss > 0 cannot be combined with the fp8 loss head (precision 'fp8' at a large vocabulary): its "
                             "e5m2 gradient scale rests on |dlogits| <= 1 / M; label_smoothing can")
        if self.fp8_head and self.ignore_index is not None:
            raise ValueError("ignore_index cannot be combined with the fp8 loss head (precision 'fp8' at a large vocabulary): its "
                             "e5m2 gradient scale rests on |dlogits| <= 1 / M, and with ignored rows the bound is 1 / N, which "
                             "only the device knows")
        self.hyper = torch.tensor([lr, betas[0], betas[1], eps, weight_decay], dtype=torch.float32, device=self.dev)
        self.hyper_host = [float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)]      # what state_dict() reports
        # lr_schedule: AdamW finds its rate in a table staged here once, by its own step word (dg_adamw_step_sched): hyper[0] is
        # not read then.  The table's address and length are launch arguments of the captured graph: set_lr_schedule() replaces
        # values, never the tensor.  no_decay: one bit per 64-float granule of flat[0, n_active); a region's alignment gap
        # belongs to its last granule (the gap holds zeros, decayed or not).
        self.lr_table = None if self.lr_table_host is None else self.lr_table_host.to(self.dev)
        self.no_decay_bits = None
        if self.no_decay:
            self.no_decay_bits = ops.new_no_decay_bits(self._no_decay_ranges(), self.n_active, self.dev)
        # what _prog_update adds to its ops.adamw_step call: nothing for an engine with neither, which then passes no keyword but
        # `clip` (a stand-in for ops.adamw_step that knows no other keeps working).  ops.adamw_step routes by what it is given.
        self._sched_kw = {}
        if self.lr_table is not None or self.no_decay_bits is not None:
            self._sched_kw = {"lr_table": self.lr_table, "no_decay_bits": self.no_decay_bits}
        # ema_decay: ema = flat[0, n_active) as the launch has just written it, averaged by AdamW's own step word (opt_state under
        # accumulation: once per optimizer step); the first step overwrites it.  ema_hyper = {decay, warmup} is read on the device:
        # set_ema_decay() writes it, captured graphs stay valid.  _ema_kw is what _prog_update adds to its
        # ops.adamw_step call: nothing for an engine without it (as _sched_kw).
        self.ema = self.ema_hyper = None
        self._ema_kw = {}
        self._in_ema = False          # inside `with ema_weights()`: flat holds the average, ema the weights
        if self.ema_decay is not None:
            self.ema = self.flat[:self.n_active].clone()
            self.ema_hyper = ops.new_ema_hyper(self.ema_decay, self.ema_warmup, self.dev)
            self._ema_kw = {"ema": self.ema, "ema_hyper": self.ema_hyper}
        # global-norm gradient clipping (ref: clip_grad_norm_(model.parameters(), max_norm) before optimizer.step()): the norm of
        # the mean gradient over ranks, gflat[0, n_active) * 1 / world, is computed inside the step and its coefficient applied
        # inside the AdamW launch; gflat / named_grads() keep the unclipped gradient.  clip_state = {total_norm, coef, max_norm, 0}
        self.max_grad_norm = None if max_grad_norm is None else check_max_grad_norm(max_grad_norm)
        self.clip_state = self.norm_work = self.last_grad_norm = None
        if self.max_grad_norm is not None:
            self.clip_state = torch.tensor([0.0, 1.0, self.max_grad_norm, 0.0], dtype=torch.float32, device=self.dev)
            self.norm_work = ops.grad_norm_workspace([self.gflat], self.dev)
            self.last_grad_norm = self.clip_state[0]          # 0-d view: the pre-clip norm of the latest step
        # the update guard: guard = {apply, total skipped, consecutive skipped, spare}, written by the finalize launch of the norm
        # (which then runs with or without clipping) and read by every workgroup of the AdamW launch; guard_limit is read on the
        # device (set_skip_grad_norm() writes it: captured graphs stay valid).  norm_out = {total_norm, coef} is clip_state where
        # the engine clips.  _guard_kw is what _prog_update adds to its ops.adamw_step call: nothing for an engine without the
        # guard (as _sched_kw).
        self.guard = self.guard_limit = self.norm_out = None
        self._guard_kw = {}
        if self.guard_on:
            self.guard = ops.new_update_guard(self.dev)
            self.guard_limit = torch.tensor([_guard_limit], dtype=torch.float32, device=self.dev)
            self.norm_out = self.clip_state
            if self.clip_state is None:
                self.norm_out = torch.zeros(2, dtype=torch.float32, device=self.dev)
                self.norm_work = ops.grad_norm_workspace([self.gflat], self.dev)
                self.last_grad_norm = self.norm_out[0]
            self._guard_kw = {"guard": self.guard}
        # dropout stream differs per data-parallel rank; the step word also drives Adam's bias correction
        self.seed = int(seed)
        self.state = ops.new_rng_state(self._rank_seed(self.seed), self.dev, 0)
        # accum_steps = k > 1: TWO counters.  state[2] becomes the micro-step word (dropout key, staged offset row, fp8 amax slot:
        # all of them move once per micro-batch; dg_grad_accumulate moves it on), opt_state[2] counts optimizer steps and is
        # AdamW's t.  gacc holds the sum of the micro-batch gradients, acc_ctl = {j, k, arrival, 0} the position inside the
        # optimizer step (_j is its host mirror), loss_acc = {sum of the micro losses, their mean after the k-th}.
        self.gacc = self.acc_ctl = self.opt_state = self.loss_acc = None
        self._j = 0
        if self.accum > 1:
            self.gacc = torch.zeros(self.n_active, dtype=torch.float32, device=self.dev)
            self.acc_ctl = ops.new_accum_ctl(self.accum, self.dev)
            self.opt_state = ops.new_rng_state(0, self.dev, 0)
            self.loss_acc = torch.zeros(2, dtype=torch.float32, device=self.dev)
        elif self.guard_on:
            # the guard with accum_steps 1: the same two words.  state[2] stays the data word (it moves every step: the AdamW
            # launch writes it through data_state), opt_state[2] is Adam's t and counts applied updates.  (accum_steps > 1:
            # dg_grad_accumulate already moves the data word.)
            self.opt_state = ops.new_rng_state(0, self.dev, 0)
            self._guard_kw["data_state"] = self.state
        # window offsets: a staged block [rows, B] the captured step walks through by itself (row = step word - off_ctl[0],
        # clamped to off_ctl[1] rows); set_offsets() is the one-row form (row 0, off_ctl[1] = 1)
        self.off_block = torch.zeros((self.OFFSET_ROWS, self.B), dtype=torch.int64, device=self.dev)
        self.offsets = self.off_block[0]
        self.off_ctl = torch.tensor([0, 1], dtype=torch.int32, device=self.dev)
        self._off_rows, self._off_left = 1, None
        self.x = torch.zeros((self.B, self.T), dtype=torch.int64, device=self.dev)
        self.y = torch.zeros((self.B, self.T), dtype=torch.int64, device=self.dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=self.dev)
        # fp8 head: dequantisation factor of the e5m2 dlogits the loss kernel writes with the a-priori scale 57344 M (|dlogits| <= 1 / M)
        self.dl_scale = torch.full((1,), 1.0 / (self.M * 57344.0), dtype=torch.float32, device=self.dev)
        self.loss_scratch = torch.zeros((2048 + 1,), dtype=torch.float32, device=self.dev)     # fused loss head: shares + arrival counter
        self.corpus: Optional[Tensor] = None
        self._graphs = None
        self._eval_graph = None
        self.force_dp_path = False      # rehearsal hook (tools/dp_rccl_smoke.py): take the multi-rank path with one rank
        self.debug_timing = False       # multi-rank step only: HIP events around backward graph(s) / exchange / optimizer graph -> last_timing (ms)
        self.last_timing: Optional[dict] = None
        self.keep_logits = False        # parity tests: keep the step's logits [M, V] alive as `last_logits` (also inside a captured graph)
        self.last_logits: Optional[Tensor] = None
        self.refresh_shadows()

    def _rank_seed(self, seed: int) -> int:
        return seed + 0x9E3779B97F4A7C15 * self.rank & 0xFFFFFFFFFFFFFFFF

    # -------------------------------------------------------------------------------- layout
    def _build_layout(self):
        C, V, L, NH, H = self.C, self.V, self.L, self.NH, self.H
        A, Bv, E, Z = _Layout(), _Layout(), _Layout(), _Layout()
        for l in range(L):
            A.add(f"{l}.wqkv", (3 * NH * H, C))
            A.add(f"{l}.wproj", (C, NH * H))
            A.add(f"{l}.w1", (4 * C, C))
            A.add(f"{l}.w2", (C, 4 * C))
        A.add("lm.w", (V, C))
        for l in range(L):
            for k, n in (("bproj", C), ("b1", 4 * C), ("b2", C), ("ln1w", C), ("ln1b", C), ("ln2w", C), ("ln2b", C)):
                Bv.add(f"{l}.{k}", (n,))
        Bv.add("lm.b", (V,))
        E.add("tok", (V, C))
        E.add("pos", (self.model.context_length, C))
        Z.add("lnf.w", (C,))
        Z.add("lnf.b", (C,))
        self.layA, self.layB, self.layE, self.layZ = A, Bv, E, Z
        self.offA, self.offB = 0, A.size
        self.offE = A.size + Bv.size
        self.n_active = self.offE + E.size           # optimizer / all-reduce range
        self.offZ = self.n_active
        self.n_total = self.n_active + Z.size

    # -------------------------------------------------------------------------------- data-parallel plan
    def _choose_buckets(self, arg: Optional[int]) -> int:
        """How many layer groups the backward pass is cut into for the gradient exchange (1 = one all-reduce of the whole flat
        gradient between the backward graph and the optimizer graph).  Bucketing overlaps the exchange of a finished group with
        the backward pass of the next one; it needs the grouped dW GEMM (bf16 mode).  Default (None, or DG_DP_BUCKETS): bucket
        when the gradient is large enough for the exchange to matter against the step -- >= 128 MB, i.e. the GPT-2 shapes
        (652 MB / 1.6 GB) -- and not for the 43 MB of the scaled model, whose whole exchange is ~0.4 ms over xGMI while every
        cut costs a graph seam and a less well filled dW launch."""
        if self.accum > 1:
            return 1
        if arg is None and os.environ.get("DG_DP_BUCKETS"):
            arg = int(os.environ["DG_DP_BUCKETS"])
        if not self.grouped_dw or (self.world == 1 and arg is None):
            return 1
        if arg is None:
            arg = 4 if self.n_active * 4 >= (128 << 20) else 1
        return max(1, min(int(arg), self.L))

    def _dp_plan(self):
        """[(layers of the group, in backward order; [(lo, hi) ranges of the flat gradient that are final after the group])].
        Region A is laid out layer 0 .. L-1 then lm_head, so a group's weight gradients are ONE contiguous range; the first group
        also carries lm_head's weight (its dW problem is the first one recorded), the last group the biases / LayerNorm vectors
        and the embeddings (B | E: contiguous, final only after the last LayerNorm backward and the embedding backward)."""
        nb, L = self.dp_buckets, self.L
        per = (L + nb - 1) // nb
        plan = []
        hi_layer = L
        while hi_layer > 0:
            lo_layer = max(0, hi_layer - per)
            lo = self.offA + self.layA.entries[f"{lo_layer}.wqkv"][0]
            hi = self.offA + (self.layA.size if hi_layer == L else self.layA.entries[f"{hi_layer}.wqkv"][0])
            ranges = [(lo, hi)]
            if lo_layer == 0:
                ranges.append((self.offB, self.n_active))
            plan.append((list(range(hi_layer - 1, lo_layer - 1, -1)), ranges))
            hi_layer = lo_layer
        return plan

    def _no_decay_ranges(self):
        """[lo, hi) element ranges of flat[0, n_active) that self.no_decay keeps out of weight decay: whole granules"""
        out = []
        for k in self._trained_keys():
            if CK.region_no_decay(k, self.no_decay):
                off, shape = self._region(k)
                out.append((off, min(_round(off + math.prod(shape)), self.n_active)))
        return out

    def _region(self, key: str):
        for lay, base in ((self.layA, self.offA), (self.layB, self.offB), (self.layE, self.offE), (self.layZ, self.offZ)):
            if key in lay.entries:
                off, shape = lay.entries[key]
                return base + off, shape
        raise KeyError(key)

    def param_view(self, key: str) -> Tensor:
        off, shape = self._region(key)
        return self.flat[off:off + math.prod(shape)].view(shape)

    def grad_view(self, key: str, buf: Optional[Tensor] = None) -> Tensor:
        off, shape = self._region(key)
        return (self.gflat if buf is None else buf)[off:off + math.prod(shape)].view(shape)

    def named_grads(self) -> Dict[str, Tensor]:
        """the step's gradient as views of the flat buffer, keyed by the reference's parameter names (what `p.grad` holds after
        `loss.backward()` in ref: src/train.py:150; after a data-parallel step: the SUM over ranks).  `ln_f.*` is absent: it never
        receives a gradient.
        accum_steps = k > 1: views of the accumulator -- the SUM over the micro-batch gradients taken so far in this optimizer
        step (all k of them after the k-th micro_step(), and over ranks after its exchange); divide by k for the mean gradient
        the optimizer applied, which is what `p.grad` holds after k x `(loss / k).backward()`."""
        buf = self.gflat if self.accum == 1 else self.gacc
        out: Dict[str, Tensor] = {}
        for name, _ in self.model.named_parameters():
            key, rows = CK.param_region(name, self.NH, self.H)
            if key not in CK.UNTRAINED:
                out[name] = CK.rows(self.grad_view(key, buf), rows)
        return out

    def _alloc_and_adopt(self):
        """copy the model's current weights into the flat buffer and re-point its Parameters at it"""
        dev, m = self.dev, self.model
        self.flat = torch.zeros(self.n_total, dtype=torch.float32, device=dev)
        self.gflat = torch.zeros(self.n_active, dtype=torch.float32, device=dev)
        self.m_ = torch.zeros(self.n_active, dtype=torch.float32, device=dev)
        self.v_ = torch.zeros(self.n_active, dtype=torch.float32, device=dev)
        # split-K workspaces of the grouped dW GEMM, one per (launch group, kind: bf16 / fp8 operands)
        self.tn_workspaces: Dict[Tuple[int, int], Tensor] = {}
        self.small_dw: Dict[str, Tuple[Tensor, int]] = {}
        # one-hot rows of the batch (bf16 [M, V rounded up to 8]): rewritten by every forward, read by the grouped dW GEMM
        self.onehot = None
        if self.grouped_dw and ops.layernorm_bwd_fused_supported(self.C) and (self.C // 4) * 8 >= S.pad_to(self.V, 8):
            self.onehot = torch.zeros((self.M, S.pad_to(self.V, 8)), dtype=torch.bfloat16, device=dev)
        if self.dp_buckets > 1:
            # bucketed step: few-tile problems leave the grouped launches (see FlatSink.matrix)
            ncu = torch.cuda.get_device_properties(dev).multi_processor_count
            for key, P, Q in (("lm.w", self.V, self.C),) + ((("tok", self.V, self.C),) if self.onehot is not None else ()):
                if ((P + 255) // 256) * ((Q + 127) // 128) <= 4:
                    n = max(1, min(64, self.M // 256, ncu // (((P + 127) // 128) * ((Q + 127) // 128))))
                    self.small_dw[key] = (torch.zeros((n, P * Q), dtype=torch.float32, device=dev), n)
        self.slabs = None if self.grouped_dw else torch.zeros((self.S, self.layA.size), dtype=torch.float32, device=dev)
        # partial rows of the bias / LayerNorm gradients: G row chunks, or as many as the GEMM epilogue that emits the column
        # sums (FeedForward's first bias) asks for; rows a producer never writes stay zero
        self.Gv = max(self.G, ops.gemm_nt_colsum_rows(self.act, self.M, 4 * self.C, self.C))
        if self.chain_bwd:
            self.Gv = max(self.Gv, 2 * (self.M // 64))            # dg_block_chain_bwd: two partial rows per 64-row block
        self.vparts = torch.zeros((self.Gv, self.layB.size), dtype=torch.float32, device=dev)
        with torch.no_grad():
            for name, param in m.named_parameters():
                key, rows = CK.param_region(name, self.NH, self.H)
                view = CK.rows(self.param_view(key), rows)
                view.copy_(param.data)
                param.data = view
        # GEMM operand shadows
        self.weights = ShadowWeights()
        self.shadow = None
        if self.act == torch.bfloat16:
            self.shadow = torch.zeros(self.n_active, dtype=torch.bfloat16, device=dev)
        self._mats: List[Tuple[Tensor, Tensor]] = []
        # every W^T lives in ONE flat buffer (like the forward shadows), so that the fp8 mode can quantise all of them with one
        # segmented launch pair
        wt_sizes = {key: shape[1] * S.k_pad(shape[0], self.act) for key, (off, shape) in self.layA.entries.items()}
        self.wt_flat = torch.zeros(sum(_round(n) for n in wt_sizes.values()), dtype=self.act, device=dev)
        seg_f, seg_b, wt_off = [], [], 0
        if self.fp8:
            self.shadow8 = torch.zeros(self.layA.size, dtype=S.E4M3, device=dev)
            self.wt8_flat = torch.zeros(self.wt_flat.numel(), dtype=S.E4M3, device=dev)
            # lm_head joins when its two contraction lengths suit the fp8 K step: K = C forward, K = V padded (50257 -> 50304 = 393 x
            # 128) in the dX direction; a char-level vocabulary (80 -> 128 columns of padding) stays bf16
            self.fp8_head = (os.environ.get("DG_FP8_HEAD", "1") != "0" and self.bf16_logits and S.fp8_k_ok(self.C) and S.fp8_k_ok(S.k_pad(self.V, self.act))
                             and self.last_block_act)
            n_fp8 = sum(1 for key in self.layA.entries if key != "lm.w" or self.fp8_head)
            self.wscale_f = torch.ones(n_fp8, dtype=torch.float32, device=dev)
            self.wscale_b = torch.ones(n_fp8, dtype=torch.float32, device=dev)
        self.wpack_flat = torch.zeros(self.layA.size, dtype=torch.bfloat16, device=dev) if (self.chain_ln or self.chain_full) else None
        self.wtpack_flat = torch.zeros(self.layA.size, dtype=torch.bfloat16, device=dev) if self.chain_bwd else None
        self._pack_pairs = []
        self._packT_pairs = []
        self._u8_pairs = []
        self.fp8_wt8 = self.fp8 and os.environ.get("DG_FP8_WT8", "1") != "0"
        for key, (off, shape) in self.layA.entries.items():
            W = self.param_view(key)
            n = shape[0] * shape[1]
            if (self.chain_ln and (key.endswith(".wproj") or key.endswith(".w2"))) or (self.chain_full and key != "lm.w"):
                pk = self.wpack_flat[off:off + n].view(shape)
                self.weights.pack_map[W.data_ptr()] = pk
                self._pack_pairs.append((self.shadow[self.offA + off:self.offA + off + n].view(shape), pk))
            if self.shadow is not None:
                self.weights.fwd_map[W.data_ptr()] = self.shadow[self.offA + off:self.offA + off + n].view(shape)
            else:
                self.weights.fwd_map[W.data_ptr()] = W
            wt_shape = (shape[1], S.k_pad(shape[0], self.act))
            Wt = self.wt_flat[wt_off:wt_off + wt_sizes[key]].view(wt_shape)
            self.weights.bwd_map[W.data_ptr()] = Wt
            self._mats.append((W, Wt))
            if self.chain_bwd and key != "lm.w":
                pkT = self.wtpack_flat[off:off + n].view(wt_shape)
                self.weights.packT_map[W.data_ptr()] = pkT
                self._packT_pairs.append((Wt, pkT))
            if self.fp8 and (key != "lm.w" or self.fp8_head):
                i = len(seg_f)
                seg_f.append([off, n])
                seg_b.append([wt_off, wt_sizes[key]])
                self.weights.fwd8_map[W.data_ptr()] = (self.shadow8[off:off + n].view(shape), self.wscale_f[i:i + 1])
                # round 3: the e4m3 W^T is the byte transposition of the e4m3 W (same values, same per-matrix scale) -- the bf16 W^T of
                # these matrices is neither refreshed nor read (DG_FP8_WT8=0: bf16 transposition + a second cast, as before)
                w8t = self.wt8_flat[wt_off:wt_off + wt_sizes[key]].view(wt_shape)
                if self.fp8_wt8:
                    self.weights.bwd8_map[W.data_ptr()] = (w8t, self.wscale_f[i:i + 1])
                    if key != "lm.w":               # (lm_head keeps its bf16 W^T too: the keep_logits / fp32-logits paths take the bf16 dX GEMM)
                        self.weights.bwd_stale.add(W.data_ptr())
                    self._u8_pairs.append((self.shadow8[off:off + n].view(shape), w8t))
                else:
                    self.weights.bwd8_map[W.data_ptr()] = (w8t, self.wscale_b[i:i + 1])
            wt_off += _round(wt_sizes[key])
        if self.fp8:
            self.seg_f = torch.tensor(seg_f, dtype=torch.int64, device=dev)
            self.seg_b = torch.tensor(seg_b, dtype=torch.int64, device=dev)
            self.w_amax = torch.zeros(len(seg_f) * ops.FP8_AMAX_PARTS, dtype=torch.float32, device=dev)

    def refresh_shadows(self):
        """bf16 copy of the GEMM weights + every W^T.  Call after the weights change outside step()
        (load_state_dict, manual edits); step() keeps them current by itself."""
        if self.shadow is not None:
            ops.cast(self.flat[:self.layA.size], torch.bfloat16, out=self.shadow[:self.layA.size])
        self._refresh_transposes()

    def _refresh_transposes(self):
        # bf16: transpose the bf16 shadow the optimizer has just written (bit-identical to casting the fp32 master, half the read)
        from_shadow = self.shadow is not None
        if getattr(self, "_tr_table", None) is None:
            pairs = [(self.weights.fwd(W) if from_shadow else W, Wt) for W, Wt in self._mats if W.data_ptr() not in self.weights.bwd_stale]
            self._tr_table = ops.make_transpose_table(pairs, self.dev) if pairs else ()
        if self._tr_table:
            ops.transpose_cast_batched(*self._tr_table, self.act, in_dtype=torch.bfloat16 if from_shadow else torch.float32)
        if self._pack_pairs:
            if getattr(self, "_pack_table", None) is None:
                self._pack_table = ops.make_pack_table(self._pack_pairs + self._packT_pairs, self.dev)
            ops.pack_chain_weights_batched(*self._pack_table)
        if self.fp8:
            # e4m3 copies of every block matrix and of every W^T, per-matrix scales: two launch pairs for the whole model
            n = self.seg_f.shape[0]
            ops.fp8_quantize(self.shadow[self.offA:self.offA + self.layA.size], S.E4M3, seg=self.seg_f, n_seg=n, out=self.shadow8,
                             scale_inv=self.wscale_f, amax=self.w_amax)
            if self.fp8_wt8:
                if getattr(self, "_u8_table", None) is None:
                    self._u8_table = ops.make_transpose_u8_table(self._u8_pairs, self.dev)
                ops.transpose_u8_batched(*self._u8_table)
            else:
                ops.fp8_quantize(self.wt_flat, S.E4M3, seg=self.seg_b, n_seg=n, out=self.wt8_flat, scale_inv=self.wscale_b, amax=self.w_amax,
                                 reuse_amax=True)          # W^T holds W's values: same per-matrix maxima, no second amax pass

    # -------------------------------------------------------------------------------- programs
    def _layer_params(self, l: int):
        pv = self.param_view
        return dict(ln1w=pv(f"{l}.ln1w"), ln1b=pv(f"{l}.ln1b"), wqkv=pv(f"{l}.wqkv"), wproj=pv(f"{l}.wproj"),
                    bproj=pv(f"{l}.bproj"), ln2w=pv(f"{l}.ln2w"), ln2b=pv(f"{l}.ln2b"), w1=pv(f"{l}.w1"), b1=pv(f"{l}.b1"),
                    w2=pv(f"{l}.w2"), b2=pv(f"{l}.b2"))

    def _forward(self, run: S.Run, x_idx: Tensor, y_idx: Optional[Tensor], want_grad: bool, gather: bool = False):
        B, T = x_idx.shape
        M = B * T
        p = self.p_drop
        # backward gets the token-table gradient as one more problem of the grouped dW GEMM: one-hot(idx)^T dx
        onehot = self.onehot if (want_grad and self.onehot is not None and M == self.M) else None
        if gather:       # get_batch inside the embedding launch: ids / targets land in self.x / self.y (= x_idx / y_idx)
            h = ops.batch_embed_fwd(self.corpus, self.off_block, self.state, self.off_ctl, x_idx, y_idx, self.param_view("tok"),
                                    self.param_view("pos"), onehot=onehot).view(M, self.C)
        else:
            h = ops.embed_fwd(x_idx, self.param_view("tok"), self.param_view("pos"), onehot=onehot).view(M, self.C)
        if self.doc_separator is not None:
            # right behind the launch that left (or read) the ids; the backward pass of this program reads the same run
            run.doc_starts = ops.doc_starts(x_idx, self.doc_separator, out=self.doc_starts if M == self.M else None)
        if self.chain_full and ops.block_chain_supported(M, self.C, self.act):
            h, saved = self._blocks_chain(run, h, B, T, want_grad)
            return self._head(run, h, y_idx, want_grad, saved, M)
        saved = []
        pre = None          # LayerNorm output for the next sub-layer, when the GEMM in front of it produced it (chain_ln)
        for l in range(self.L):
            P = self._layer_params(l)
            nxt = [] if self.chain_ln else None
            h, sa = S.attn_fwd(run, h, P["ln1w"], P["ln1b"], P["wqkv"], P["wproj"], P["bproj"], True, B, T, self.NH, self.H, p, p, l,
                               pre=pre, fuse_ln=(P["ln2w"], P["ln2b"]) if self.chain_ln else None, nxt=nxt)
            pre = nxt[0] if nxt else None
            last = l == self.L - 1
            nxt = [] if (self.chain_ln and not last) else None
            Pn = self._layer_params(l + 1) if nxt is not None else None
            h, sf = S.ffn_fwd(run, h, P["ln2w"], P["ln2b"], P["w1"], P["b1"], P["w2"], P["b2"], True, p, l,
                              out_dtype=self.act if (last and self.last_block_act) else torch.float32,
                              pre=pre, fuse_ln=(Pn["ln1w"], Pn["ln1b"]) if nxt is not None else None, nxt=nxt)
            pre = nxt[0] if nxt else None
            if want_grad:
                saved.append((sa, sf))
        return self._head(run, h, y_idx, want_grad, saved, M)

    def _blocks_chain(self, run: S.Run, h: Tensor, B: int, T: int, want_grad: bool):
        """the residual blocks with everything between two attention calls in ONE launch (dg_block_chain_fwd): head (LayerNorm 1 +
        QKV of block 0), then per block attention + chain (proj .. the next block's QKV; the last block stops behind its second
        residual add and hands lm_head a bf16 tensor).  Leaves exactly the tensors the separate launches leave for backward."""
        M, C = h.shape
        p = run.p(self.p_drop)
        pk = self.weights.pack
        saved = []
        P = self._layer_params(0)
        r = ops.block_chain_fwd(2, M, C, x=h, ln1w=P["ln1w"], ln1b=P["ln1b"], wqkv=pk(P["wqkv"]))
        x, h1, m1, r1, qkv = h, r["h1"], r["mean1"], r["rstd1"], r["qkv"]
        for l in range(self.L):
            o, lse = ops.attn_fwd(qkv, B, T, self.NH, self.H, self.H ** -0.5, p, run.rng, S.site_attn(l), keep=want_grad,
                                  doc_starts=run.doc_starts)
            last = l == self.L - 1
            if self.chain_warm:
                # the layer's packed weight stream (wproj | w1 | w2 | the next block's wqkv: contiguous in the packed buffer)
                lo = self.layA.entries[f"{l}.wproj"][0]
                hi = self.layA.entries[f"{l + 1}.wproj"][0] if not last else self.layA.entries["lm.w"][0]
                ops.l2_warm(self.wpack_flat[lo:hi])
            kw = dict(o=o, x=x, wproj=pk(P["wproj"]), bproj=P["bproj"], ln2w=P["ln2w"], ln2b=P["ln2b"], w1=pk(P["w1"]), b1=P["b1"],
                      w2=pk(P["w2"]), b2=P["b2"], dropout_p=p, rng_state=run.rng, site_proj=S.site_proj(l), site_ffn=S.site_ffn(l))
            if last:
                r = ops.block_chain_fwd(1, M, C, **kw)
            else:
                Pn = self._layer_params(l + 1)
                r = ops.block_chain_fwd(0, M, C, ln1w=Pn["ln1w"], ln1b=Pn["ln1b"], wqkv=pk(Pn["wqkv"]), **kw)
            if want_grad:
                saved.append(((x, h1, m1, r1, qkv, o, lse), (r["x1"], r["h2"], r["mean2"], r["rstd2"], r["f"], r["bits"])))
            x = r["x2"]
            if not last:
                P, h1, m1, r1, qkv = Pn, r["h1"], r["mean1"], r["rstd1"], r["qkv"]
        return x, saved

    def _head(self, run: S.Run, h: Tensor, y_idx: Optional[Tensor], want_grad: bool, saved, M: int):
        okw = self._loss_kw if want_grad else {}        # the objective's options: training programs only, evaluation stays plain
        gs = 1.0 / M
        if self.ignore_index is not None and y_idx is not None:
            # the targets' option, in training and evaluation alike: count the rows that count (after the gather that may have
            # drawn them), hand the kernels 1 / N on the device
            ops.count_valid(y_idx.view(M), self.ignore_index, out=self.token_count)
            okw = dict(okw, ignore_index=self.ignore_index, inv_count=self.token_count[1:])
            gs = 1.0
        if self.bf16_logits and y_idx is not None and not self.keep_logits:
            # large vocabulary: lm_head writes bf16 logits into the buffer that becomes dlogits -- the cross-entropy kernel holds
            # a whole row in registers and overwrites it in place with its gradient (1.65 GB less written and 0.82 GB less read
            # per step at the GPT-2 vocabulary, M = 8192, than fp32 logits + a separate bf16 gradient)
            buf = torch.empty((M, S.k_pad(self.V, self.act)), dtype=self.act, device=self.dev)
            if self.fp8_head and run.fp8 and h.dtype == torch.bfloat16:
                # precision fp8 (round 3): lm_head's three contractions on the fp8 MFMA too.  Forward on e4m3 x e4m3; the loss kernel
                # leaves its gradient a second time as e5m2 (a-priori scale: |dlogits| <= 1 / M) -- operand of the dX GEMM and of the
                # weight gradient (the bf16 gradient in `buf` still feeds the bias column sums)
                Wl = self.param_view("lm.w")
                xq, xs = S._quantize_operand(run, h, S.E4M3, "lm.x")
                h.dg_fp8x = (xq, xs)
                wq, ws = self.weights.fwd8(Wl)
                logits = ops.gemm_nt(xq, wq, self.act, scale_a=xs, scale_b=ws, bias=self.param_view("lm.b"), out=buf[:, :self.V])
                if want_grad and M == self.M:
                    q8 = torch.empty((M, buf.shape[1]), dtype=S.E5M2, device=self.dev)
                    rows = ops.cross_entropy_fp8(logits, y_idx.view(M), self.V, buf, gs, q8, **okw)      # (z_loss, ignore_index: refused at construction)
                    buf.dg_q8 = (q8, self.dl_scale)
                else:
                    rows = ops.cross_entropy(logits, y_idx.view(M), self.V, dlogits=buf if want_grad else None, grad_scale=gs, **okw)
                return None, rows, (saved, h, buf)
            logits, (xa,) = S.linear_fwd(run, h, self.param_view("lm.w"), self.param_view("lm.b"), out=buf[:, :self.V])
            rows = ops.cross_entropy(logits, y_idx.view(M), self.V, dlogits=buf if want_grad else None, grad_scale=gs, **okw)
            return None, rows, (saved, xa, buf)
        logits, (xa,) = S.linear_fwd(run, h, self.param_view("lm.w"), self.param_view("lm.b"), pad_rows=True)
        if y_idx is None:
            return logits, None, None
        dlogits = None
        if want_grad:
            dlogits = torch.empty((M, S.k_pad(self.V, self.act)), dtype=self.act, device=self.dev)
            if M == self.M and ops.cross_entropy_fused_supported(logits, dlogits, self.G):
                # small vocabulary: the loss head in one launch -- gradient rows, the lm_head bias partials and the mean loss
                part, stride, n = FlatSink(self).vector("lm.b", self.V)
                rows = ops.cross_entropy_fused(logits, y_idx.view(M), self.V, dlogits, gs, part, stride, n, self.loss_scratch,
                                               self.loss, gs, **okw)
                return logits, rows, (saved, xa, dlogits, True)
        rows = ops.cross_entropy(logits, y_idx.view(M), self.V, dlogits=dlogits, grad_scale=gs, **okw)
        return logits, rows, (saved, xa, dlogits)

    def _backward_begin(self, run: S.Run, x_idx: Tensor, ctx) -> dict:
        saved, xa, dlogits = ctx[:3]
        head_done = len(ctx) > 3            # the fused loss head already left the lm_head bias partials (and the loss) behind
        st = dict(run=run, x_idx=x_idx, saved=saved, sink=FlatSink(self), g_next=None, g0=None)
        g = dlogits[:, :self.V]
        q8 = getattr(dlogits, "dg_q8", None)
        if q8 is not None:
            g.dg_fp8 = (q8[0][:, :self.V], q8[1])          # the e5m2 copy the loss kernel left (fp8 head)
        st["dh"] = S.linear_bwd_from_act(run, (xa,), g, self.param_view("lm.w"), True, st["sink"], {"w": "lm.w", "b": "lm.b"},
                                         bias_done=head_done)
        return st

    def _backward_layers(self, st: dict, layers) -> None:
        """backward of the given blocks (descending).  st["g_next"]: dropout-backward of dh for the sub-layer that runs next,
        fused into the LayerNorm backward that produced dh"""
        run, sink, saved, x_idx = st["run"], st["sink"], st["saved"], st["x_idx"]
        B, T = x_idx.shape
        p = self.p_drop
        dh, g_next = st["dh"], st["g_next"]
        for l in layers:
            P = self._layer_params(l)
            sa, sf = saved[l]
            dh, g_next = S.ffn_bwd(run, sf, dh, P["ln2w"], P["w1"], P["w2"], True, p, l, sink,
                                   {"w1": f"{l}.w1", "b1": f"{l}.b1", "w2": f"{l}.w2", "b2": f"{l}.b2", "ln_w": f"{l}.ln2w", "ln_b": f"{l}.ln2b"},
                                   g_in=g_next, emit=(p, S.site_proj(l), f"{l}.bproj", self.C, f"{l}.g_proj"))
            keys = {"wqkv": f"{l}.wqkv", "wproj": f"{l}.wproj", "bproj": f"{l}.bproj", "ln_w": f"{l}.ln1w", "ln_b": f"{l}.ln1b"}
            if l > 0:
                dh, g_next = S.attn_bwd(run, sa, dh, P["ln1w"], P["wqkv"], P["wproj"], True, B, T, self.NH, self.H, p, p, l, sink, keys,
                                        g_in=g_next, emit=(p, S.site_ffn(l - 1), f"{l - 1}.b2", self.C, f"{l - 1}.g_ffn"))
            elif self.onehot is not None:
                # first block: also take dx in bf16 (no dropout, no bias behind it) -- the X operand of the token-table problem
                dh, st["g0"] = S.attn_bwd(run, sa, dh, P["ln1w"], P["wqkv"], P["wproj"], True, B, T, self.NH, self.H, p, p, l, sink, keys,
                                          g_in=g_next, emit=(0.0, 0, None, self.C))
            elif self.stream_dtype != torch.float32:
                # (bf16 gradient stream: the fused LayerNorm backward is the only form that writes it; its g output is unused)
                dh, _ = S.attn_bwd(run, sa, dh, P["ln1w"], P["wqkv"], P["wproj"], True, B, T, self.NH, self.H, p, p, l, sink, keys,
                                   g_in=g_next, emit=(0.0, 0, None, self.C))
            else:
                dh = S.attn_bwd(run, sa, dh, P["ln1w"], P["wqkv"], P["wproj"], True, B, T, self.NH, self.H, p, p, l, sink, keys, g_in=g_next)
        st["dh"], st["g_next"] = dh, g_next

    def _backward_layers_chain(self, st: dict) -> None:
        """backward of all residual blocks with everything between two attention-backward calls in ONE launch (dg_block_chain_bwd):
        the top block's second half (mode 1), per block boundary the first half of block l + the second half of block l - 1 (mode 0),
        block 0's first half (mode 2).  Records the same (dY, X) operand pairs for the grouped dW launch and writes the same partial
        rows of the bias / LayerNorm gradients (two per 64-row block) as the separate launches."""
        run, sink, saved, x_idx = st["run"], st["sink"], st["saved"], st["x_idx"]
        B, T = x_idx.shape
        M, C, L = self.M, self.C, self.L
        p = run.p(self.p_drop)
        pkT = self.weights.packT
        stride = self.layB.size

        def vec(key, n):
            return sink.vector(key, n)[0]

        def second(l):
            P = self._layer_params(l)
            x1, h2, mean2, rstd2, f, bits = saved[l][1]
            return dict(w2T=pkT(P["w2"]), bits=bits, db1_part=vec(f"{l}.b1", 4 * C), w1T=pkT(P["w1"]), x1=x1, mean2=mean2, rstd2=rstd2,
                        ln2w=P["ln2w"], dln2w_part=vec(f"{l}.ln2w", C), dln2b_part=vec(f"{l}.ln2b", C), gbias2_part=vec(f"{l}.bproj", C),
                        wprojT=pkT(P["wproj"]), site_proj=S.site_proj(l))

        def first(l, dqkv, dresid):
            P = self._layer_params(l)
            x, h1, m1, r1, qkv, o, lse = saved[l][0]
            return dict(dqkv=dqkv, wqkvT=pkT(P["wqkv"]), x=x, mean1=m1, rstd1=r1, ln1w=P["ln1w"], dresid1=dresid,
                        dln1w_part=vec(f"{l}.ln1w", C), dln1b_part=vec(f"{l}.ln1b", C),
                        gbias1_part=vec(f"{l - 1}.b2", C) if l > 0 else None, site_ffn_below=S.site_ffn(l - 1) if l > 0 else 0)

        def weights_and_attention(l, g, r):
            """the four weight-gradient problems of block l and its attention backward; returns dqkv"""
            x, h1, m1, r1, qkv, o, lse = saved[l][0]
            x1, h2, mean2, rstd2, f, bits = saved[l][1]
            S.weight_grad(sink, f"{l}.w2", g, f, C, 4 * C)
            S.weight_grad(sink, f"{l}.w1", r["df"], h2, 4 * C, C)
            S.weight_grad(sink, f"{l}.wproj", r["g2"], o, C, C)
            dqkv = ops.attn_bwd(qkv, o, r["dout"], lse, B, T, self.NH, self.H, self.H ** -0.5, p, run.rng, S.site_attn(l),
                                doc_starts=run.doc_starts)
            S.weight_grad(sink, f"{l}.wqkv", dqkv, h1, 3 * C, C)
            return dqkv

        kw = dict(part_stride=stride, dropout_p=p, rng_state=run.rng)
        dh = st["dh"]
        l = L - 1
        part, pstride, n = sink.vector(f"{l}.b2", C)
        g = ops.dropout_bwd_cast(dh, run.act, p, run.rng, S.site_ffn(l), colsum_part=part, part_stride=pstride, n_partials=n)
        r = ops.block_chain_bwd(1, M, C, g_in=g, dresid2=dh, **second(l), **kw)
        while True:
            dqkv = weights_and_attention(l, g, r)
            if l == 0:
                break
            r = ops.block_chain_bwd(0, M, C, **first(l, dqkv, r["dx2"]), **second(l - 1), **kw)
            g = r["g1"]
            l -= 1
        r = ops.block_chain_bwd(2, M, C, **first(0, dqkv, r["dx2"]), **kw)
        st["dh"], st["g0"], st["g_next"] = r["dx1"], r["g1"], None

    def _backward_end(self, st: dict, group: int = 0) -> None:
        x_idx, dh, sink = st["x_idx"], st["dh"], st["sink"]
        B, T = x_idx.shape
        if self.onehot is not None:
            S.weight_grad(sink, "tok", self.onehot[:, :self.V], st["g0"], self.V, self.C)
            ops.embed_bwd(x_idx, dh.view(B, T, self.C), None, self.grad_view("pos")[:T], V=self.V)
        else:
            ops.embed_bwd(x_idx, dh.view(B, T, self.C), self.grad_view("tok"), self.grad_view("pos")[:T])
        if self.grouped_dw:
            sink.flush(group)
        else:
            ops.reduce_partials(self.slabs, self.layA.size, self.S, self.gflat[self.offA:], self.layA.size)
        ops.reduce_partials(self.vparts, self.layB.size, self.Gv, self.gflat[self.offB:], self.layB.size)

    def _train_run(self) -> S.Run:
        """per-step runtime configuration of the training program.  fp8: every quantisation site keeps its amax history in
        self.fp8_sites (one-pass delayed scaling); the first execution (the eager warm-up before capture, or the first eager
        step) quantises just in time and seeds the history"""
        seed = self.fp8 and not self._fp8_seeded
        if seed:
            self._fp8_seeded = True
        return S.Run(act=self.act, rng=self.state if self.p_drop > 0.0 else None, weights=self.weights, fp8=self.fp8, split=self.split_bf16,
                     fp8_sites=self.fp8_sites if self.fp8 else None, fp8_seed=seed, step_word=self.state, stream=self.stream_dtype,
                     fp8_only=self.fp8 and self.fp8_dw and self.grouped_dw and os.environ.get("DG_FP8_ONLY", "1") != "0")

    def _mean_rows(self, rows: Tensor, out: Optional[Tensor] = None) -> Tensor:
        """the mean of a loss head's rows: over all of them, or with ignore_index over the N that count (the count it just left)"""
        if self.ignore_index is None:
            return ops.reduce_sum(rows, 1.0 / rows.numel(), out=out)
        return ops.reduce_sum(rows, 1.0, out=out, scale_dev=self.token_count[1:])

    @property
    def last_token_count(self) -> Optional[Tensor]:
        """ignore_index: N, the targets that counted in the last loss head that ran (0-d device view; reading it synchronises)"""
        return None if self.token_count is None else self.token_count[0]

    def _prog_front(self) -> dict:
        """gather the batch, forward, the loss, lm_head's backward: the step up to the backward pass of the residual blocks"""
        run = self._train_run()
        logits, rows, ctx = self._forward(run, self.x, self.y, True, gather=self.corpus is not None)
        if self.keep_logits:
            self.last_logits = logits
        if len(ctx) == 3:
            self._mean_rows(rows, self.loss)
        return self._backward_begin(run, self.x, ctx)

    def _prog_fwd_bwd(self):
        """gather the batch, forward, backward, reduce the gradient partials"""
        st = self._prog_front()
        if self.chain_bwd:
            self._backward_layers_chain(st)
        else:
            self._backward_layers(st, reversed(range(self.L)))
        self._backward_end(st)

    def _prog_segments(self):
        """[(segment, ranges)]: the same step cut at the layer-group boundaries of _dp_plan().  Segment k ends with the grouped dW
        launch of its group, after which the group's ranges of the flat gradient are final and their all-reduce can start"""
        plan = self._dp_plan()
        st = {}

        def seg(k, layers):
            if k == 0:
                st.clear()
                st.update(self._prog_front())
            self._backward_layers(st, layers)
            if k == len(plan) - 1:
                self._backward_end(st, group=k)
                st.clear()                      # release the activations (they live in the graph pool anyway)
            else:
                st["sink"].flush(k)

        return [(functools.partial(seg, k, layers), ranges) for k, (layers, ranges) in enumerate(plan)]

    def _prog_micro(self):
        """accum_steps > 1: one micro-batch -- the step's forward / backward, then its gradient and loss into the accumulators; that
        launch also moves the micro-step word on (nothing behind it reads the word)"""
        self._prog_fwd_bwd()
        ops.grad_accumulate(self.gacc, self.gflat, self.n_active, self.acc_ctl, self.loss, self.loss_acc, self.state)

    def _prog_update(self):
        """norm (if clipping or guarded), AdamW, W^T refresh.  The gradient is final here on every path (the data-parallel update runs after
        the exchange): gflat * 1 / world, the mean over ranks, with the step word as t -- or, accum_steps = k > 1, gacc * 1 /
        (k * world), the mean over micro-batches and ranks, with the optimizer's own counter.  The word moves on inside the AdamW
        launch: nothing after it reads the word."""
        grad = self.gflat if self.accum == 1 else self.gacc
        word = self.state if self.opt_state is None else self.opt_state
        scale = 1.0 / (self.accum * self.world)
        clip = {}
        if self.guard is not None:
            # the guard: the norm's two launches with or without clipping; the finalize launch also decides whether AdamW applies
            # the update (norm <= limit, and -- one rank -- the step's loss finite: under accumulation the running sum of the micro
            # losses).  With more ranks the all-reduced gradient alone decides, so that every rank decides the same.
            loss = None if self.world > 1 else (self.loss if self.accum == 1 else self.loss_acc[0:1])
            ops.grad_norm(grad, scale, None if self.clip_state is None else self.clip_state[2:3], self.norm_out, self.norm_work,
                          guard=self.guard, limit=self.guard_limit, loss=loss)
            if self.clip_state is not None:
                clip = {"clip": self.clip_state[1:2]}
        elif self.clip_state is not None:
            # AdamW on g * coef.  The alignment gaps of the gradient buffer are zero (no producer writes them), so the norm over
            # the whole active range is the norm over the parameters.
            ops.grad_norm(grad, scale, self.clip_state[2:3], self.clip_state, self.norm_work)
            clip = {"clip": self.clip_state[1:2]}
        ops.adamw_step(self.flat, grad, self.m_, self.v_, self.hyper, word, scale, shadow_bf16=self.shadow, n=self.n_active,
                       advance=True, **clip, **self._sched_kw, **self._ema_kw, **self._guard_kw)
        self._refresh_transposes()

    # -------------------------------------------------------------------------------- the step: description, capture, run
    def _dp(self) -> bool:
        return self.world > 1 or self.force_dp_path

    def _step_programs(self):
        """the optimizer step as ([(backward program, the exchange behind it)], update program).  The exchange is None, WHOLE, or
        the [(lo, hi)] ranges of the flat gradient a layer group has finished (all-reduced asynchronously beside the next group).
        accum_steps = k: the micro program k times, the exchange behind the last.  Everything that runs a step -- eagerly, as the
        warm-up before capture, to seed the fp8 histories, captured -- runs this."""
        if self._dp() and self.dp_buckets > 1:
            backward = self._prog_segments()
        elif self.accum > 1:
            backward = [(self._prog_micro, None)] * (self.accum - 1) + [(self._prog_micro, WHOLE)]
        else:
            backward = [(self._prog_fwd_bwd, WHOLE)]
        return backward, self._prog_update

    def _snapshot(self):
        """copy every buffer and counter the step's programs move; returns the call that puts them back"""
        bufs = [self.flat, self.m_, self.v_, self.state]
        bufs += [b for b in (self.ema, self.gacc, self.acc_ctl, self.opt_state, self.loss_acc, self.guard) if b is not None]
        snap = [b.clone() for b in bufs]

        def put_back():
            for b, c in zip(bufs, snap):
                b.copy_(c)
        return put_back

    def _capture(self):
        """one graph per distinct program of the step, all in one pool (the multi-rank step and accumulation: the exchange runs
        between replays) -- or the whole step in ONE graph: a single process with accum_steps 1.  The warm-up runs every program
        once, in step order; what it moved is put back before the capture.  Sets _graphs and _replay: the step description with
        every program replaced by its graph's replay (the one-graph step: no backward stages, the whole step in the update slot)."""
        backward, update = self._step_programs()
        progs = list(dict.fromkeys(p for p, _ in backward)) + [update]
        one_graph = not self._dp() and self.accum == 1
        if one_graph:
            def whole_step(parts=tuple(progs)):
                for p in parts:
                    p()
            progs = [whole_step]
        put_back, hist = self._snapshot(), self._fp8_snapshot()

        def restore():
            put_back()
            self._fp8_put_back(hist)
            self.refresh_shadows()

        self._graphs = capture_after_warmup(self.dev, progs, restore)
        if one_graph:
            self._replay = [], self._graphs[0].replay
        else:
            replay = dict(zip(progs, (g.replay for g in self._graphs)))
            self._replay = [(replay[p], exchange) for p, exchange in backward], replay[update]

    def _exchange(self, exchange, works: list) -> None:
        """the SUM all-reduce behind a backward program; the mean is the 1 / world inside AdamW.  WHOLE: the whole gradient buffer
        (accum_steps > 1: the accumulated gradient, once per optimizer step), synchronously.  Ranges: each one asynchronously --
        RCCL enqueues it on its own stream behind the work already submitted to the current stream (the segment that produced
        the ranges) and it then runs beside the next segment; `works` are joined before the update."""
        import torch.distributed as dist
        if exchange is WHOLE:
            dist.all_reduce(self.gflat if self.accum == 1 else self.gacc, op=dist.ReduceOp.SUM, group=self.pg)
        else:
            for lo, hi in exchange:
                works.append(dist.all_reduce(self.gflat[lo:hi], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))

    def _run(self, lo: Optional[int] = None, hi: Optional[int] = None) -> None:
        """run the backward stages [lo, hi) of the step (default: all of them) -- the programs themselves, or (use_graph) their
        graphs' replay -- and, behind the step's last stage, the exchange's join and the update"""
        if not self.use_graph:
            backward, update = self._step_programs()
        else:
            if self._graphs is None:
                self._capture()
            backward, update = self._replay
        stages = backward[lo:hi]
        last = hi is None or hi >= len(backward)
        dp = last and self._dp()
        whole = dp and stages[-1][1] is WHOLE           # (only ever behind the step's last backward stage)
        ev = self._timing_events(3) if (dp and self.use_graph and self.accum == 1) else None
        works = []
        for prog, exchange in stages:
            prog()
            if dp and isinstance(exchange, list):
                self._exchange(exchange, works)
        if ev: ev[1].record()
        if whole:
            self._exchange(WHOLE, works)
        for w in works:
            w.wait()                    # stream-level join with the RCCL stream (no host block with the nccl backend)
        if ev: ev[2].record()
        if last:
            update()
        if ev:
            self._timing_done(ev, ("backward_graphs", "exposed_exchange", "optimizer_graph") if self.dp_buckets > 1 else
                              ("backward_graph", "exchange", "optimizer_graph"))

    # -------------------------------------------------------------------------------- public
    def set_corpus(self, data: Tensor):
        """keep the token stream resident in HBM (int64, as train_data.pt stores it)"""
        if data.dim() != 1 or data.numel() < self.T + 1:
            raise ValueError(f"set_corpus: need a 1-D token stream of more than context_length = {self.T} tokens")
        self.corpus = data.to(self.dev, dtype=torch.int64).contiguous()
        ops.check_ids(self.corpus, self.V, "the corpus")          # once, here: the captured step never checks
        self._graphs = None

    def set_lr(self, lr: float):
        if self.lr_table is not None:
            raise RuntimeError("set_lr: this engine follows a learning-rate schedule (TrainEngine(..., lr_schedule=...)); "
                               "set_lr_schedule() replaces its values")
        self.hyper_host[0] = float(lr)
        self.hyper[0:1].fill_(float(lr))

    def set_lr_schedule(self, values, schedule_steps: Optional[int] = None):
        """new values for the staged table, from the next step on (a device copy: captured graphs stay valid).  The table's
        length is fixed at construction: ValueError for another one, RuntimeError on an engine built without a schedule."""
        if self.lr_table is None:
            raise RuntimeError("set_lr_schedule: this engine was built without a schedule (TrainEngine(..., lr_schedule=...))")
        table = SCH.as_table(values, schedule_steps)
        if table.numel() != self.lr_table.numel():
            raise ValueError(f"set_lr_schedule: the new schedule has {table.numel()} entries, this engine's table has "
                             f"{self.lr_table.numel()} (the length is fixed at construction)")
        self.lr_table_host = table
        self.lr_table.copy_(table)

    def current_lr(self) -> float:
        """the rate the next optimizer step uses: table[min(step_count(), len - 1)], or the constant rate without a schedule.
        Synchronises on an engine with a schedule."""
        if self.lr_table_host is None:
            return self.hyper_host[0]
        return float(self.lr_table_host[min(self.step_count(), self.lr_table_host.numel() - 1)])

    def set_max_grad_norm(self, max_norm: float):
        """a new clipping threshold for the following steps (a device write: captured graphs stay valid)"""
        if self.clip_state is None:
            raise RuntimeError("set_max_grad_norm: this engine was built without clipping (TrainEngine(..., max_grad_norm=...))")
        self.max_grad_norm = check_max_grad_norm(max_norm)
        self.clip_state[2:3].fill_(self.max_grad_norm)

    # ---- the update guard (TrainEngine(skip_nonfinite=..., skip_grad_norm=...))
    def _need_guard(self, what: str) -> None:
        if self.guard is None:
            raise RuntimeError(f"{what}: this engine was built without the update guard (TrainEngine(..., skip_nonfinite=True) or "
                               "skip_grad_norm=...)")

    def set_skip_grad_norm(self, limit: Optional[float]):
        """a new norm limit for the following steps, or None for non-finite gradients only (a device write: captured graphs stay
        valid)"""
        self._need_guard("set_skip_grad_norm")
        staged = ops.check_guard_options(True, limit)[1]
        self.skip_grad_norm = None if limit is None else staged
        self.guard_limit.fill_(staged)

    @property
    def last_step_applied(self) -> Optional[Tensor]:
        """1 if the latest optimizer step applied its update, 0 if the guard skipped it (0-d device view; reading it synchronises;
        None without the guard)"""
        return None if self.guard is None else self.guard[0]

    def skipped_steps(self) -> int:
        """optimizer steps the guard has skipped so far.  Synchronises."""
        self._need_guard("skipped_steps")
        return int(self.guard[1].item()) & 0xFFFFFFFF

    def consecutive_skips(self) -> int:
        """optimizer steps skipped in a row up to the latest one (0 after an applied update).  Synchronises."""
        self._need_guard("consecutive_skips")
        return int(self.guard[2].item()) & 0xFFFFFFFF

    # ---- the moving average of the weights (TrainEngine(ema_decay=...))
    def _refuse_in_ema(self, what: str) -> None:
        if self._in_ema:
            raise RuntimeError(f"{what} inside `with ema_weights()`: the weights are swapped with their moving average; leave the "
                               "context first")

    def _need_ema(self, what: str) -> None:
        if self.ema is None:
            raise RuntimeError(f"{what}: this engine was built without a moving average (TrainEngine(..., ema_decay=...))")

    def set_ema_decay(self, decay: float):
        """a new decay for the following optimizer steps (a device write: captured graphs stay valid)"""
        self._need_ema("set_ema_decay")
        d = ops.check_ema_options(decay, self.ema_warmup)
        if d is None:
            raise ValueError("set_ema_decay: the decay must be a number in (0, 1); an engine cannot drop its moving average")
        self.ema_decay = d
        self.ema_hyper[0:1].fill_(d)

    def ema_view(self, key: str) -> Tensor:
        """the moving average of one trained region, a view of `ema` (as param_view is a view of `flat`)"""
        self._need_ema("ema_view")
        return self.grad_view(key, self.ema)

    def ema_state_dict(self) -> dict:
        """the moving average in the model's state_dict() format, as CPU tensors: loads into a plain TransformerLM.  The per-head
        query / key / value entries are rows of the packed QKV region (the mapping of optimizer_state_dict); tensors the engine
        does not train (ln_f) are the model's.  Synchronises."""
        self._need_ema("ema_state_dict")
        self._refuse_in_ema("ema_state_dict()")
        img = self.ema.cpu()
        out = {}
        for name, t in self.model.state_dict().items():
            try:
                key, rows = CK.param_region(name, self.NH, self.H)
            except KeyError:
                key = None
            if key is None or key in CK.UNTRAINED:
                out[name] = t.detach().cpu().clone()
            else:
                out[name] = CK.rows(self.grad_view(key, img), rows).clone()
        return out

    def _swap_ema(self) -> None:
        ops.swap_(self.flat, self.ema, self.n_active)
        if self.shadow is not None:      # (the optimizer launch keeps the whole bf16 image current; refresh_shadows() the GEMM weights)
            lo = self.layA.size
            ops.cast(self.flat[lo:self.n_active], torch.bfloat16, out=self.shadow[lo:])
        self.refresh_shadows()

    @contextlib.contextmanager
    def ema_weights(self):
        """`with engine.ema_weights():` -- evaluate, sample or export the averaged weights.  On entry the weights and their moving
        average change places (one dg_swap_f32 launch) and every weight-derived copy is rebuilt from them (refresh_shadows); the
        model's Parameters are views of `flat` and captured graphs hold its address, so eval_loss, eval_losses, model.generate and
        model.state_dict() all see the average.  On exit the same again: the derived copies are functions of the weights alone,
        so training continues bit for bit.  Inside, whatever would train on or save the swapped buffers raises RuntimeError."""
        self._need_ema("ema_weights")
        self._refuse_in_ema("ema_weights()")
        if self._j:
            raise RuntimeError(f"ema_weights(): {self._j} of {self.accum} micro-steps of the current optimizer step are taken; finish "
                               "it with micro_step() first")
        self._swap_ema()
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._swap_ema()

    def set_offsets(self, ix: Tensor):
        """window offsets of THIS rank's rows for the next step (drawn by the host CPU generator, ref: preprocessing.py:43)"""
        if self._off_rows != 1:
            self.off_ctl[1:2].fill_(1)
            self._off_rows, self._off_left = 1, None
        if ix.is_cuda:
            self.offsets.copy_(ix, non_blocking=True)      # stream-ordered device copy (range-checked where they were staged)
        else:
            self.check_offsets(ix)
            self.offsets.copy_(ix)                         # synchronous: stage blocks of offsets instead (stage_offsets)

    def stage_offsets(self, block: Tensor):
        """window offsets of the next block.shape[0] steps, [n, B] (host tensors are range-checked, device tensors are taken as
        checked): step k after this call gathers row k by itself -- the captured step reads its row from the device-side step
        counter, so a training loop is nothing but graph launches between two stagings"""
        if block.dim() != 2 or block.shape[1] != self.B or block.shape[0] < 1:
            raise ValueError(f"stage_offsets: need [n >= 1, B = {self.B}] offsets")
        if self.accum > 1:
            # one row per micro-step: optimizer step s after this call consumes rows s * k .. s * k + k - 1
            if block.shape[0] % self.accum:
                raise ValueError(f"stage_offsets: {block.shape[0]} rows are no multiple of accum_steps = {self.accum}")
            if self._j:
                raise RuntimeError(f"stage_offsets: {self._j} of {self.accum} micro-steps of the current optimizer step are taken; "
                                   "finish it with micro_step() first")
        if not block.is_cuda:
            self.check_offsets(block)
        n = block.shape[0]
        self._grow_offsets(n)
        self.off_block[:n].copy_(block, non_blocking=block.is_cuda)
        self.off_ctl[0:1].copy_(self.state[2:3])          # device-side: row = step word - step word now
        self.off_ctl[1:2].fill_(n)
        self._off_rows, self._off_left = n, n

    def _grow_offsets(self, n: int) -> None:
        if n > self.off_block.shape[0]:
            # a larger block buffer is a new address: captured graphs go (and with them the view set_offsets writes)
            self.off_block = torch.zeros((n, self.B), dtype=torch.int64, device=self.dev)
            self.offsets = self.off_block[0]
            self._graphs = None

    def _take_offset_rows(self, what: str, n: int = 1) -> None:
        if self._off_left is not None:
            if self._off_left <= 0:
                raise RuntimeError(f"{what}: the {self._off_rows} staged offset rows are used up; stage_offsets() or set_offsets() first")
            self._off_left -= n

    def check_offsets(self, ix: Tensor):
        """window offsets must leave room for T + 1 tokens (ref: randint(len(data) - context_length), src/preprocessing.py:43);
        host tensors are checked for free, device tensors cost one round trip: check a staged block once, not every step"""
        if self.corpus is not None and ix.numel():
            lo, hi = (int(v) for v in torch.aminmax(ix))
            if lo < 0 or hi + self.T + 1 > self.corpus.numel():
                raise IndexError(f"window offsets in [{lo}, {hi}] do not fit a corpus of {self.corpus.numel()} tokens at T = {self.T}")

    def set_batch(self, x: Tensor, y: Tensor):
        """token / target ids of this rank's rows, given directly (ids are validated here; the captured step never checks)"""
        ops.check_ids(x, self.V, "x")
        if self.ignore_index is None:
            ops.check_ids(y, self.V, "y")
        else:
            ops.check_ids(y, self.V, "y", allow=self.ignore_index)
        self.x.copy_(x, non_blocking=True)
        self.y.copy_(y, non_blocking=True)

    def micro_step(self) -> Tensor:
        """one micro-batch on the current offsets / batch: forward, backward, its gradient added into the accumulator; returns the
        micro-batch's loss (device scalar).  The accum_steps-th call also runs the gradient exchange (one all-reduce of the
        accumulated gradient) and the optimizer update on the mean gradient.  accum_steps == 1: the same as step()."""
        self._refuse_in_ema("micro_step()")
        if self.accum == 1:
            return self.step()
        self._take_offset_rows("micro_step()")
        self._run(self._j, self._j + 1)
        self._j = (self._j + 1) % self.accum
        return self.loss

    def step(self) -> Tensor:
        """one training iteration on the current offsets / batch; returns the device loss scalar.  accum_steps = k > 1: k
        micro-steps on the next k staged offset rows and one optimizer update; returns the mean of their losses."""
        self._refuse_in_ema("step()")
        k = self.accum
        if k > 1:
            if self.corpus is None or self._off_left is None:
                raise RuntimeError(f"step() with accum_steps = {k} runs {k} micro-batches and needs {k} staged offset rows "
                                   "(set_corpus + stage_offsets); with batches given by set_batch() / set_offsets() call micro_step() "
                                   "once per batch -- step() would use the same batch for every micro-step")
            if self._j:
                raise RuntimeError(f"step(): {self._j} of {k} micro-steps of the current optimizer step are taken; finish it with micro_step()")
            if self._off_left < k:
                raise RuntimeError(f"step(): {self._off_left} of the {self._off_rows} staged offset rows are left, one optimizer step "
                                   f"needs {k}; stage_offsets() first")
        self._take_offset_rows("step()", k)
        self._run()
        return self.loss if k == 1 else self.loss_acc[1]

    def _timing_events(self, n: int):
        if not self.debug_timing:
            return None
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
        ev[0].record()
        return ev

    def _timing_done(self, ev, names) -> None:
        """debug_timing: where a multi-rank step spends its time (one host sync; never on in a timed run)"""
        if ev:
            ev[-1].record()
            ev[-1].synchronize()
            self.last_timing = {n: ev[i].elapsed_time(ev[i + 1]) for i, n in enumerate(names)}

    @torch.no_grad()
    def eval_loss(self, x: Tensor, y: Tensor) -> Tensor:
        """forward only, dropout off (ref: evaluate_loss, src/train.py:61-75)"""
        run = S.Run(act=self.act, rng=None, weights=self.weights, fp8=self.fp8, split=self.split_bf16)
        _, rows, _ = self._forward(run, x, y, False)
        return self._mean_rows(rows)

    @torch.no_grad()
    def eval_losses(self, data: Tensor, offsets: Tensor) -> Tensor:
        """losses of offsets.shape[0] forward-only batches (dropout off) drawn from the resident token stream `data` at the
        window offsets `offsets` [n, B] (int64, on the device): the inner loop of evaluate_loss (ref: src/train.py:66-72)
        as one gather launch + one captured forward graph per batch and no host synchronisation; returns [n] on the device.
        Eagerly it was ~55 ctypes launches and a `.item()` per batch -- more host time than the 0.85 ms the GPU needs."""
        n, B = offsets.shape
        if B != self.B:
            raise ValueError(f"eval_losses: batches of {B} rows, the engine was built for {self.B}")
        out = torch.empty(n, dtype=torch.float32, device=self.dev)
        if not self.use_graph:
            for i in range(n):
                x, y = ops.batch_gather(data, offsets[i], self.T)
                out[i:i + 1].copy_(self.eval_loss(x, y).view(1))
            return out
        if self._eval_graph is None:
            self.ev_x = torch.zeros((self.B, self.T), dtype=torch.int64, device=self.dev)
            self.ev_y = torch.zeros((self.B, self.T), dtype=torch.int64, device=self.dev)
            self.ev_loss = torch.zeros(1, dtype=torch.float32, device=self.dev)

            def prog():
                run = S.Run(act=self.act, rng=None, weights=self.weights, fp8=self.fp8, split=self.split_bf16)
                _, rows, _ = self._forward(run, self.ev_x, self.ev_y, False)
                self._mean_rows(rows, self.ev_loss)
            self._eval_graph, = capture_after_warmup(self.dev, [prog])
        for i in range(n):
            ops.batch_gather(data, offsets[i], self.T, self.ev_x, self.ev_y)
            self._eval_graph.replay()
            out[i:i + 1].copy_(self.ev_loss)
        return out

    # -------------------------------------------------------------------------------- training state
    _LOSS_FIELDS = ("label_smoothing", "z_loss")

    def _meta(self) -> dict:
        meta = {"precision": str(self.model.precision), "vocab_size": int(self.V), "embedding_dim": int(self.C), "num_layers": int(self.L),
                "num_heads": int(self.NH), "model_context_length": int(self.model.context_length), "batch_size": self.B,
                "context_length": self.T, "accum_steps": self.accum, "world_size": int(self.world), "dropout": self.p_drop}
        meta.update(self._loss_kw)      # only where set: a default engine writes and accepts exactly the files it always did
        if self.ignore_index is not None:
            meta["ignore_index"] = self.ignore_index
        if getattr(self, "doc_separator", None) is not None:
            meta["doc_separator"] = self.doc_separator
        if self.ema is not None:
            meta["ema"] = True
        if self.guard is not None:
            meta["update_guard"] = True
        return meta

    def _check_meta(self, saved: dict) -> None:
        """CK.check_compat on the fields every engine has; the loss options in both directions (a field absent on either side reads
        as 0.0: a smoothed state is refused by a default engine as much as the reverse)"""
        CK.check_compat(saved, {k: v for k, v in self._meta().items() if k not in self._LOSS_FIELDS and k not in ("ema", "ignore_index", "update_guard", "doc_separator")})
        CK.check_ema_meta(saved, self.ema is not None)
        CK.check_guard_meta(saved, self.guard is not None)
        for field in self._LOSS_FIELDS:
            theirs, own = saved.get(field, 0.0), self._loss_kw.get(field, 0.0)
            if isinstance(theirs, bool) or not isinstance(theirs, (int, float)) or float(theirs) != own:
                raise ValueError(f"training state: meta.{field} differs: saved {theirs!r}, this run has {own!r}")
        theirs = saved.get("ignore_index")
        if isinstance(theirs, bool) or not (theirs is None or isinstance(theirs, int)) or theirs != self.ignore_index:
            raise ValueError(f"training state: meta.ignore_index differs: saved {theirs!r}, this run has {self.ignore_index!r}")
        # the document mask changes no state: a file written without it loads into an engine with it and the other way round;
        # two separators are compared
        theirs, own = saved.get("doc_separator"), getattr(self, "doc_separator", None)
        if theirs is not None and own is not None and (isinstance(theirs, bool) or not isinstance(theirs, int) or theirs != own):
            raise ValueError(f"training state: meta.doc_separator differs: saved {theirs!r}, this run has {own!r}")

    def _param_names(self) -> List[str]:
        return [n for n, _ in self.model.named_parameters()]

    def _trained_keys(self) -> List[str]:
        return [k for lay in (self.layA, self.layB, self.layE) for k in lay.entries]

    def _fp8_snapshot(self):
        """capture warm-up of an engine whose fp8 histories are loaded state: they are put back like flat / m_ / v_ / state (a
        fresh engine's warm-up SEEDS them, and keeps what it seeded)"""
        if not (self.fp8 and self._fp8_keep and self._fp8_seeded):
            return None
        return {k: v.clone() for k, v in self.fp8_sites.items()}

    def _fp8_put_back(self, snap) -> None:
        if snap:
            for k, v in snap.items():
                self.fp8_sites[k].copy_(v)

    def is_finite(self) -> bool:
        """are the weights and Adam's moments all finite?  The sum-of-squares launch of the gradient norm over flat, m_ and v_ and
        one device round trip: ask before a good checkpoint is replaced by a diverged run's."""
        if self._finite_work is None:
            self._finite_work = ops.grad_norm_workspace([self.flat, self.m_, self.v_], self.dev)
        return ops.all_finite([self.flat, self.m_, self.v_], self._finite_work)

    def optimizer_state_dict(self) -> dict:
        """Adam's state in torch.optim.AdamW's own format, as AdamW(model.parameters(), ...) would save it after step_count()
        steps (CPU tensors; the per-head query / key / value moments are rows of the packed QKV region; ln_f has no entry;
        before the first step `state` is empty, as torch's is).  Synchronises."""
        step = self.step_count()
        regions = {}
        if step > 0:
            m, v = self.m_.cpu(), self.v_.cpu()
            regions = {k: (self.grad_view(k, m), self.grad_view(k, v)) for k in self._trained_keys()}
        h = self.hyper_host
        lr = h[0] if self.lr_table_host is None else float(self.lr_table_host[min(step, self.lr_table_host.numel() - 1)])
        return CK.optimizer_state_from_regions(self._param_names(), regions, self.NH, self.H, step, lr, (h[1], h[2]), h[3], h[4],
                                               no_decay=self.no_decay)

    def _parse_optimizer_state(self, sd: dict):
        """validate an optimizer state_dict against this engine; returns (m, v as CPU images of the flat buffers, step, hyper)"""
        try:
            regions, step, hyper = CK.regions_from_optimizer_state(sd, self._param_names(), self.NH, self.H, no_decay=self.no_decay)
        except KeyError as e:
            raise ValueError(f"optimizer state: missing key {e}") from None
        keys = self._trained_keys()
        for k in regions:
            if k not in keys:
                raise ValueError(f"optimizer state: {k} is not a trained region of this engine")
        if step > 0 and set(regions) != set(keys):
            raise ValueError(f"optimizer state: no moments for {sorted(set(keys) - set(regions))}")
        m = torch.zeros(self.n_active, dtype=torch.float32)
        v = torch.zeros(self.n_active, dtype=torch.float32)
        for k, (rm, rv) in regions.items():
            shape = self._region(k)[1]
            if tuple(rm.shape) != shape or tuple(rv.shape) != shape:
                raise ValueError(f"optimizer state: {k} has shape {tuple(rm.shape)}, this engine's is {shape}")
            self.grad_view(k, m).copy_(rm)
            self.grad_view(k, v).copy_(rv)
        if not 0 <= step < (1 << 32):
            raise ValueError(f"optimizer state: step count {step} does not fit the device-side step word")
        return m, v, step, hyper

    def _write_optimizer_state(self, m: Tensor, v: Tensor, step: int, hyper: dict) -> None:
        self.m_.copy_(m)
        self.v_.copy_(v)
        self.hyper_host = [hyper["lr"], hyper["betas"][0], hyper["betas"][1], hyper["eps"], hyper["weight_decay"]]
        self.hyper.copy_(torch.tensor(self.hyper_host, dtype=torch.float32))
        word = self.state if self.opt_state is None else self.opt_state
        word[2:3].copy_(ops.new_rng_state(0, self.dev, step)[2:3])

    @torch.no_grad()
    def load_optimizer_state_dict(self, sd: dict) -> None:
        """moments, step count and hyper-parameters from optimizer_state_dict(), torch.optim.AdamW or drakegpt_amd.optim.AdamW over
        the same model, written in place (captured graphs stay valid).  ValueError if the parameters disagree about the step
        count or the state does not fit.  accum_steps == 1: the step word also keys dropout and selects the staged offset row,
        so loading another step count moves those too -- load_state_dict() is the form that keeps every counter consistent."""
        self._refuse_in_ema("load_optimizer_state_dict()")
        m, v, step, hyper = self._parse_optimizer_state(sd)
        self._write_optimizer_state(m, v, step, hyper)

    def state_dict(self) -> dict:
        """everything a following step reads that an earlier step or call wrote, as CPU tensors and plain values (DESIGN.md
        section 4 lists every buffer).  Synchronises; not for the hot path.  RuntimeError inside an optimizer step."""
        self._refuse_in_ema("state_dict()")
        if self._j:
            raise RuntimeError(f"state_dict(): {self._j} of {self.accum} micro-steps of the current optimizer step are taken; finish it "
                               "with micro_step() first (a half-filled gradient accumulator is not a state to save)")
        torch.cuda.synchronize(self.dev)
        used = 0 if self._off_left is None else self._off_rows - self._off_left
        eng = {"seed": self.seed, "step_word": int(self.state[2].item()) & 0xFFFFFFFF,
               "opt_step": None if self.accum == 1 else int(self.opt_state[2].item()) & 0xFFFFFFFF,
               "acc_ctl": None if self.accum == 1 else self.acc_ctl.cpu(),
               "max_grad_norm": self.max_grad_norm,
               "offsets": self.off_block[used:self._off_rows].cpu(), "offsets_rows": self._off_rows, "offsets_left": self._off_left,
               "fp8_seeded": bool(self._fp8_seeded),
               "fp8_sites": {k: v.cpu() for k, v in self.fp8_sites.items()} if self.fp8 else {},
               "lr_table": None if self.lr_table_host is None else self.lr_table_host.clone(), "no_decay": list(self.no_decay)}
        if self.ema is not None:
            eng["ema"] = {"decay": self.ema_decay, "warmup": self.ema_warmup, "values": self.ema.cpu()}
        if self.guard is not None:      # only where on: a default engine writes exactly the files it always did
            eng["guard"] = {"skipped": self.skipped_steps(), "consecutive": self.consecutive_skips(), "limit": self.skip_grad_norm,
                            "opt_step": int(self.opt_state[2].item()) & 0xFFFFFFFF}
        return {"format": CK.FORMAT, "version": CK.VERSION,
                "model": {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                "optimizer": self.optimizer_state_dict(), "engine": eng, "meta": self._meta()}

    _ENGINE_KEYS = ("seed", "step_word", "opt_step", "acc_ctl", "max_grad_norm", "offsets", "offsets_rows", "offsets_left",
                    "fp8_seeded", "fp8_sites")

    @torch.no_grad()
    def load_state_dict(self, sd: dict) -> None:
        """continue the run state_dict() was taken from: the next step() is the step that run would have taken next.  Everything is
        validated before anything is written (ValueError names the field and both values; the engine is untouched then), and
        written in place: the model's Parameters stay views of `flat` and captured graphs stay valid (a staged block larger than
        the offset buffer is the one exception, as in stage_offsets).  Hyper-parameters follow the file; clipping on / off follows
        this engine, its threshold the file where both clip.  The update guard: a file written with it restores both step words,
        both counters and the limit; a file written without it loads into a guarded engine (the optimizer word starts at the
        step word, the counters at 0); a guarded file is refused by an engine without the guard.  Every rank loads rank 0's file; the dropout stream is re-derived
        from the saved seed for this rank.  precision fp8: a rank other than 0 seeds its amax histories afresh."""
        self._refuse_in_ema("load_state_dict()")
        CK.check_format(sd)
        for k in ("model", "optimizer", "engine", "meta"):
            if k not in sd:
                raise ValueError(f"training state: missing key {k!r}")
        self._check_meta(sd["meta"])
        e = sd["engine"]
        for k in self._ENGINE_KEYS:
            if k not in e:
                raise ValueError(f"training state: missing key engine.{k}")
        own = self.model.state_dict()
        for k, t in own.items():
            if k not in sd["model"]:
                raise ValueError(f"training state: missing key model.{k}")
            if tuple(sd["model"][k].shape) != tuple(t.shape):
                raise ValueError(f"training state: model.{k} has shape {tuple(sd['model'][k].shape)}, this model's is {tuple(t.shape)}")
        for k in sd["model"]:
            if k not in own:
                raise ValueError(f"training state: model.{k} is not a tensor of this model")
        # (a file written before schedules and decay groups existed has neither key: no schedule, no groups)
        table, groups = e.get("lr_table"), e.get("no_decay") or []
        own_len = None if self.lr_table_host is None else self.lr_table_host.numel()
        if table is not None and (not isinstance(table, Tensor) or table.dim() != 1 or table.dtype != torch.float32):
            raise ValueError("training state: engine.lr_table is not a 1-D float32 tensor")
        saved_len = None if table is None else table.numel()
        if saved_len != own_len:
            raise ValueError(f"training state: engine.lr_table differs: saved {saved_len!r} entries, this engine's schedule has "
                             f"{own_len!r} (None: no schedule)")
        if table is not None:
            try:
                table = SCH.as_table(table)
            except ValueError as err:
                raise ValueError(f"training state: engine.lr_table: {err}") from None
        if sorted(groups) != list(self.no_decay):
            raise ValueError(f"training state: engine.no_decay differs: saved {sorted(groups)!r}, this engine has {list(self.no_decay)!r}")
        ema_sd = CK.check_ema_state(e.get("ema"), self.ema is not None, self.n_active)
        m, v, step, hyper = self._parse_optimizer_state(sd["optimizer"])
        word = int(e["step_word"])
        opt_step = word if self.accum == 1 else e["opt_step"]
        # the update guard: a guarded file restores both words, both counters and the limit; an unguarded file into a guarded
        # engine starts the optimizer word at the step word and the counters at 0 (the guard can be turned on mid-run); a guarded
        # file into an engine without the guard was refused by _check_meta
        guard_sd = CK.check_guard_state(e.get("guard"), sd["meta"], self.guard is not None, word)
        if guard_sd is not None and guard_sd[4]:
            if self.accum > 1 and e["opt_step"] != guard_sd[0]:
                raise ValueError(f"training state: engine.guard.opt_step is {guard_sd[0]}, engine.opt_step {e['opt_step']!r}")
            opt_step = guard_sd[0]
        if opt_step is None or int(opt_step) != step:
            raise ValueError(f"training state: engine step count differs: the engine section says {opt_step!r}, the optimizer state {step}")
        if self.accum > 1:
            ctl = e["acc_ctl"]
            if ctl is None or tuple(ctl.shape) != (4,) or ctl.dtype != torch.int32 or ctl.tolist()[:2] != [0, self.accum]:
                raise ValueError(f"training state: engine.acc_ctl is {None if ctl is None else ctl.tolist()!r}, this engine needs "
                                 f"[0, {self.accum}, ...] (saved between two optimizer steps)")
        left, rows, offs = e["offsets_left"], int(e["offsets_rows"]), e["offsets"]
        n = 1 if left is None else int(left)
        if offs.dim() != 2 or offs.dtype != torch.int64 or tuple(offs.shape) != (n, self.B) or not 0 <= n <= max(rows, 1):
            raise ValueError(f"training state: engine.offsets is {tuple(offs.shape)} {offs.dtype}, expected {(n, self.B)} int64 "
                             f"({left!r} of {rows} staged rows left)")
        if self.corpus is not None and n:
            lo, hi = (int(x) for x in torch.aminmax(offs))
            if lo < 0 or hi + self.T + 1 > self.corpus.numel():
                raise ValueError(f"training state: engine.offsets in [{lo}, {hi}] do not fit this engine's corpus of "
                                 f"{self.corpus.numel()} tokens at T = {self.T}")
        mgn = e["max_grad_norm"]
        if mgn is not None and self.clip_state is not None:
            try:
                mgn = check_max_grad_norm(mgn)
            except ValueError as err:
                raise ValueError(f"training state: engine.{err}") from None
        sites = None
        if self.fp8 and self.rank == 0 and e["fp8_seeded"]:
            sites = e["fp8_sites"]
            if not self._fp8_seeded:
                # the histories do not exist before the first execution: run the step's backward programs once, as a fresh engine's
                # warm-up does, so that they exist to be written.  accum_steps 1: that writes the gradient buffers and the loss,
                # scratch.  accum_steps > 1: the micro program's accumulate launch also moves gacc, acc_ctl, loss_acc and the
                # micro-step word, which are put back
                put_back = self._snapshot() if self.accum > 1 else None
                for prog in dict.fromkeys(p for p, _ in self._step_programs()[0]):
                    prog()
                if put_back is not None:
                    put_back()
                torch.cuda.synchronize(self.dev)
            for k, t in self.fp8_sites.items():
                if k not in sites:
                    raise ValueError(f"training state: missing key engine.fp8_sites.{k}")
                if tuple(sites[k].shape) != tuple(t.shape):
                    raise ValueError(f"training state: engine.fp8_sites.{k} has shape {tuple(sites[k].shape)}, this engine's is {tuple(t.shape)}")
        # ---- nothing was written up to here (but scratch); from here on nothing fails
        for k, t in own.items():
            t.copy_(sd["model"][k])
        self._write_optimizer_state(m, v, step, hyper)
        if table is not None:
            self.lr_table_host = table
            self.lr_table.copy_(table)
        if ema_sd is not None:
            self.ema_decay, self.ema_warmup = ema_sd[0], ema_sd[1]
            self.ema_hyper.copy_(torch.tensor([self.ema_decay, 1.0 if self.ema_warmup else 0.0], dtype=torch.float32))
            self.ema.copy_(ema_sd[2])
        self.seed = int(e["seed"])
        self.state.copy_(ops.new_rng_state(self._rank_seed(self.seed), self.dev, word))
        if self.opt_state is not None:
            self.opt_state[2:3].copy_(ops.new_rng_state(0, self.dev, step)[2:3])
        if self.accum > 1:
            self.acc_ctl.copy_(e["acc_ctl"])
        if guard_sd is not None:
            # (apply, the latest decision, follows from the consecutive count)
            self.guard.copy_(torch.tensor([0 if guard_sd[2] else 1, *(x - (1 << 32) if x >= (1 << 31) else x for x in guard_sd[1:3]), 0],
                                          dtype=torch.int32))
            if guard_sd[4]:
                self.set_skip_grad_norm(guard_sd[3])
        self._j = 0
        if mgn is not None and self.clip_state is not None:
            self.set_max_grad_norm(mgn)
        self._grow_offsets(n)
        if n:
            self.off_block[:n].copy_(offs)
        self.off_ctl.copy_(torch.tensor([word - (1 << 32) if word >= (1 << 31) else word, max(n, 1)], dtype=torch.int32))
        self._off_rows, self._off_left = (1, None) if left is None else (n if n else rows, n)
        if self.fp8:
            if sites is not None:
                for k, t in self.fp8_sites.items():
                    t.copy_(sites[k])
                self._fp8_keep = True
            elif self._fp8_seeded:
                # (a rank other than 0, or a file saved before its first step) seed again, as a fresh engine does: the seeding
                # execution makes new history tensors, so graphs that hold the old ones go
                self._fp8_seeded, self._fp8_keep = False, False
                self.fp8_sites.clear()
                self._graphs = None
        if self.shadow is not None:      # (the optimizer launch keeps the whole bf16 image current; refresh_shadows() the GEMM weights)
            ops.cast(self.flat[:self.n_active], torch.bfloat16, out=self.shadow)
        self.refresh_shadows()

    def check_status(self) -> None:
        """raise if a bounded device-side wait of the grouped dW GEMM ever ran out (dg_gemm_tn_grouped: the sticky error word in
        the last 16 bytes of its workspace).  One device round trip: for tests / end-of-run checks, not for every step."""
        for ws in self.tn_workspaces.values():
            if int(ws[-16:].view(torch.int32)[0].item()) != 0:
                raise RuntimeError("dg_gemm_tn_grouped: a split-K hand-over timed out; weight gradients since then are invalid")

    def step_count(self) -> int:
        """optimizer steps taken (with the update guard: updates applied)"""
        return int((self.state if self.opt_state is None else self.opt_state)[2].item())

    def micro_step_count(self) -> int:
        """micro-batches run: the word that keys dropout and selects the staged offset row (== step_count() for accum_steps 1)"""
        return int(self.state[2].item())
