"""Graph-replayed decoding for TransformerLM.generate(sampler="device") -- ref: src/model.py:611-636.

The training step is one graph launch that walks a device-side step counter; generation gets the same shape here.  The decode
state {seed_lo, seed_hi, L, 0} lives on the device (L = current sequence length), every kernel of a step reads its position from
it, the sampler writes token L into the ids buffer and dg_state_advance moves L on.  Two linear chains are captured once per
(batch, device, precision) and replayed once per token, with no host work in between:

  graph A (K/V-cached step, valid while L <= ctx): embed_window mode 0, per layer LN / QKV GEMM into a staging row /
      attn_decode_append / proj / LN / FFN, lm_head, sample_rows, state_advance
  graph B (sliding-window step, valid for L >= ctx): embed_window mode 1, the eval forward kernels at T = ctx
      (TransformerLM._forward_rows), lm_head on the last row, sample_rows, state_advance
      Both walk the model's one layer stack (TransformerLM._layers); graph A passes it the attention step above.

Graphs hold raw pointers, so the decoder owns every operand: staged copies of the weights (refreshed on every generate call),
the K/V caches, the ids buffer, the state and the sampler parameters (always the four-word block of dg_sample_rows_nucleus:
temperature, top_k, top_p and min_p change between calls without a new capture).

A call with a penalty, a logit bias or a stop token replays a second pair of graphs, captured on the first such call: the same
two chains ending in dg_sample_rows_control.  Its operands are the decoder's too -- the 16-word control block, bias [V], the
token counts [B, V] that the kernel keeps up to date and lengths [B], the rows' "finished" state that the next replay honours --
and every call that uses them rewrites all four first.  A call without controls replays the first pair, as it always did.

A call with prompt_lengths (rows that start at different lengths) replays a third pair, captured on the first such call: the same
two chains ending in dg_sample_rows_ragged, which reads one more operand of the decoder's, spans [B, 2], rewritten by every such
call with the other four.  The shared position L starts at the shortest prompt; a row still inside its prompt is left alone by
the sampler and reads its next prompt token from ids like any other token.  Which pair a call uses is its mode (MODES); the
tail, the capture and the step are written once and take it as an argument.

A call that asks for log-probabilities (return_logprobs, top_logprobs, best_of) replays the scored twin of its mode's pair,
captured on the first such call per mode: the same two chains with one dg_token_logprobs launch between the sampler and
dg_state_advance, which scores the token just written at ids[:, L] into the decoder's result buffers (logprobs [B, cap], top ids
and top log-probabilities [B, cap, 20]) and skips the rows that lengths and spans mark as finished or forced.  begin_scores()
refills the buffers and sets the top_n word outside the graphs.  A call without those arguments replays the unscored pairs.
"""
from __future__ import annotations

import weakref

import torch

from . import ops
from .engine import capture_after_warmup
from .model import ControlOperands


MODES = ("plain", "control", "ragged")          # the sampler entry a step ends in: nucleus, control, ragged


class DeviceDecoder:
    def __init__(self, model, B: int, device, min_cap: int):
        ctx = model.context_length
        C = model.token_embedding_table.weight.shape[1]
        self.B, self.ctx, self.C = B, ctx, C
        self.NH, self.H = model._heads()
        self.act, self.split = model.act_dtype, model.split_bf16
        self.device = device
        self._mref = weakref.ref(model)          # the model owns the decoder, not the other way round
        # the ids row length is a launch argument of the captured kernels: round the capacity up so that calls of similar length
        # share one capture
        self.cap = max(ctx + 1, (min_cap + 255) // 256 * 256)
        self.ids = torch.zeros((B, self.cap), dtype=torch.int64, device=device)
        self.state = torch.zeros(4, dtype=torch.int32, device=device)
        # four words {inv_temp, top_k, top_p, min_p}: the captured sampler is dg_sample_rows_nucleus, whatever the call asks for
        self.params = ops.new_sample_params(1.0, None, device, four=True)
        self.caches = [torch.zeros((B, ctx, 3 * C), dtype=self.act, device=device) for _ in model.blocks]
        self.row = torch.zeros((B, 3 * C), dtype=self.act, device=device)       # staging: the new token's q/k/v
        self.ws = self.w_lm = self.tok = self.pos = self.lm_bias = None
        self.pairs = {}          # mode -> (graph A, graph B), each captured on the first call in that mode
        # scored twins (generate(return_logprobs= / top_logprobs= / best_of=)): the same steps with one dg_token_logprobs launch
        # between the sampler and dg_state_advance, captured on the first scored call per mode; their result buffers are the
        # decoder's, made with the first of them
        self.pairs_scored = {}
        self.scores = self.top_n = None          # (logprobs [B, cap], top_ids [B, cap, 20], top_logprobs [B, cap, 20]), the top_n word
        # the operands of dg_sample_rows_control, the tail of the second pair of graphs (captured on the first call that asks for a
        # penalty, a bias or a stop token): every call that uses them rewrites all four first (ControlOperands.begin); a call with
        # prompt_lengths (the third pair, dg_sample_rows_ragged) rewrites spans with them
        self.operands = ControlOperands(B, model.token_embedding_table.weight.shape[0], device, spans=True)
        self.control, self.bias, self.counts, self.lengths = self.operands.kw().values()
        self.spans = self.operands.spans

    graphs = property(lambda self: self.pairs.get("plain"))
    graphs_control = property(lambda self: self.pairs.get("control"))
    graphs_ragged = property(lambda self: self.pairs.get("ragged"))

    # ------------------------------------------------------------------ operands
    @torch.no_grad()
    def refresh(self, model) -> None:
        """copy the model's current weights into the staged operands (allocated on the first call)"""
        ws, w_lm = model._decode_weights()
        src = [t for W in ws for t in W.values()] + [w_lm, model.token_embedding_table.weight,
                                                     model.position_embedding_table.weight, model.lm_head.bias]
        if self.ws is None:
            own = [t.detach().clone() for t in src]
            n = len(ws[0])
            keys = list(ws[0].keys())
            self.ws = [dict(zip(keys, own[l * n:(l + 1) * n])) for l in range(len(ws))]
            self.w_lm, self.tok, self.pos, self.lm_bias = own[len(ws) * n:]
            self._flat = own
        else:
            for d, s in zip(self._flat, src):
                d.copy_(s)

    @torch.no_grad()
    def begin_scores(self, top_n: int) -> None:
        """the start of a scored call, outside the graphs: logprobs zero-filled, top_* sentinel-filled (-1 / -inf) -- the launches
        write the scored positions and nothing else -- and the top_n word the kernel reads (allocated on the first call)"""
        if self.scores is None:
            from .model import new_score_buffers
            self.scores = new_score_buffers(self.B, self.cap, self.device)
            self.top_n = torch.zeros(1, dtype=torch.int32, device=self.device)
        else:
            self.scores[0].zero_()
            self.scores[1].fill_(-1)
            self.scores[2].fill_(float("-inf"))
        self.top_n.fill_(int(top_n))

    # ------------------------------------------------------------------ the two steps
    def tail(self, logits, mode: str = "plain", scored: bool = False) -> None:
        """sample (control / ragged: dg_sample_rows_control / dg_sample_rows_ragged on the decoder's operands) and advance;
        scored: in between, dg_token_logprobs on the token just placed at ids[:, L] -- it skips the rows that the mode's lengths
        and spans mark as finished or forced"""
        assert mode in MODES, mode
        ops.sample_rows(logits, self.state, self.params, ids=self.ids, **({} if mode == "plain" else self.operands.kw(mode == "ragged")))
        if scored:
            ops.token_logprobs(logits, self.ids, state=self.state, lengths=None if mode == "plain" else self.lengths,
                               spans=self.spans if mode == "ragged" else None, out=self.scores[0], out_top_ids=self.scores[1],
                               out_top_lp=self.scores[2], top_n=self.top_n)
        ops.state_advance(self.state)

    def _step_cached(self, model, mode: str, scored: bool = False) -> None:
        """TransformerLM._decode_step at the device position L - 1"""
        def attend(l, h, wqkv):
            ops.gemm_nt(h, wqkv, self.act, out=self.row, split=self.split)
            return ops.attn_decode_append(self.row, self.caches[l], self.state, self.NH, self.H, self.H ** -0.5)

        x = ops.embed_window(self.ids, self.state, self.tok, self.pos, 0)
        self.tail(model._lm_logits(model._layers(x, self.ws, attend), self.w_lm, self.lm_bias), mode, scored)

    def _step_window(self, model, mode: str, scored: bool = False) -> None:
        """the full forward on the last ctx tokens (the reference algorithm once the window slides)"""
        x = ops.embed_window(self.ids, self.state, self.tok, self.pos, 1).view(self.B * self.ctx, self.C)
        self.tail(model._forward_rows(x, self.B, self.ctx, None, self.ws, self.w_lm, self.lm_bias), mode, scored)

    # ------------------------------------------------------------------ capture / replay
    @torch.no_grad()
    def capture(self, mode: str = "plain", scored: bool = False) -> None:
        """capture both steps of `mode` once, each after a warm-up run at its own position (engine.capture_after_warmup; the state
        word is put back in between).  A warm-up step writes cache row L - 1 and ids[:, L]: the call that follows writes its prompt
        into ids after the capture, and the real step at that L rewrites both before anything reads them.  "control": the second
        pair, the same steps ending in dg_sample_rows_control; its warm-up also touches counts and lengths, which
        ControlOperands.begin rewrites before every use.  "ragged": the third pair, ending in dg_sample_rows_ragged; its warm-up
        runs on whatever spans hold (any values are safe: they only pick which rows sample), and begin rewrites them too.
        scored: the mode's scored twins, into pairs_scored; their warm-up writes columns 1 and ctx of the score buffers, which
        begin_scores refills before every use.  The unscored pair of the mode is neither needed nor touched."""
        pairs = self.pairs_scored if scored else self.pairs
        if mode in pairs:
            return
        if scored and self.scores is None:
            self.begin_scores(0)
        model = self._mref()
        graphs = []
        for L, step in ((1, self._step_cached), (self.ctx, self._step_window)):
            def position(L=L):
                self.state.copy_(ops.new_rng_state(0, self.device, step=L))
            position()
            graphs += capture_after_warmup(self.device, [lambda step=step: step(model, mode, scored)], position)
        pairs[mode] = tuple(graphs)

    def step(self, cached: bool, graph: bool = True, mode: str = "plain", scored: bool = False) -> None:
        if graph:
            (self.pairs_scored if scored else self.pairs)[mode][0 if cached else 1].replay()
        else:
            (self._step_cached if cached else self._step_window)(self._mref(), mode, scored)
