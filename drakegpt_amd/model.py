"""The six DrakeGPT language models on the gfx950 HIP kernels.

Mirror of the reference's src/model.py: same class names, constructor signatures, attribute and
state_dict layout, ``forward(idx, targets=None) -> (logits, loss)`` (logits flattened to (B*T, V)
when targets are given, src/model.py:601-609) and ``generate(idx, max_new_tokens)``.

Reference quirks kept on purpose:
  * TransformerLM owns ``ln_f`` but never applies it (src/model.py:572,598-599): the parameters
    exist in the state_dict, take no part in compute and never receive a gradient;
  * MultiHeadAttentionLM's per-head size is head_size // num_heads (src/model.py:264);
  * generate() crops to context_length (src/model.py:625) and samples from torch's CPU generator so that, given
    matching logits, the sampled indices are bit-identical to the reference run on CPU.  The five earlier-stage
    models re-run the full forward per token as the reference does; TransformerLM.generate keeps a K/V cache while
    the sequence fits the context window (same logits, see its docstring) and falls back to the reference
    algorithm once the window slides;
  * token / target ids outside [0, vocab_size) raise IndexError at the module boundary, as nn.Embedding and
    F.cross_entropy do in the reference (the kernels themselves clamp and never fault).
"""
from __future__ import annotations

import math
import numbers
from collections import OrderedDict
from typing import NamedTuple, Optional

import torch
import torch.nn as nn
from torch import Tensor

from . import functional as HF
from . import ops
from .model_component import (Block, Head, HipModule, MultiHeadAttention, ResidualBlock, ResidualBlock2)


def model_params(params: dict, model_type: str, vocab_size: int) -> int:
    """The reference's parameter-count ESTIMATE (src/model.py:8-63), reproduced because train.py
    prints it (src/train.py:112-113).  It is not the true count; use
    ``sum(p.numel() for p in model.parameters())`` for that."""
    C, T, L = params["embedding_dim"], params["context_length"], params["num_layers"]
    kqv = 3 * C * C
    attention = C + kqv + C * C
    ffw = C * 4 * C
    mlp = C + 2 * ffw
    total = C * vocab_size
    if model_type != "BigramLM":
        total += C * T + kqv + C * vocab_size
    if model_type in ("SingleHeadAttentionLM", "MultiHeadAttentionLM"):
        total += C * T + C * vocab_size
    if model_type == "BlocksLM":
        total += (kqv + ffw) * L
    if model_type == "ResidualBlocksLM":
        total += (kqv + 2 * ffw) * L
    if model_type == "TransformerLM":
        total += (attention + mlp) * L + vocab_size
    return total


def check_sampling_args(sampler, temperature, top_k, vocab_size: int):
    """the argument checks of generate(): plain Python, raised before anything touches a device.  Returns (temperature as a
    float, top_k clamped to the vocabulary or None)."""
    if sampler not in ("host", "device"):
        raise ValueError(f"generate: sampler must be 'host' or 'device', got {sampler!r}")
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"generate: temperature must be a number, got {temperature!r}") from None
    if not math.isfinite(t) or t < 0.0:
        raise ValueError(f"generate: temperature must be finite and >= 0, got {temperature!r}")
    if top_k is not None:
        if isinstance(top_k, bool) or int(top_k) != top_k or top_k < 1:
            raise ValueError(f"generate: top_k must be an integer >= 1 (or None), got {top_k!r}")
        top_k = min(int(top_k), int(vocab_size))
    return t, top_k


def _number(x, name) -> float:
    if isinstance(x, bool):
        raise ValueError(f"generate: {name} must be a number, got {x!r}")
    try:
        return float(x)
    except (TypeError, ValueError):
        raise ValueError(f"generate: {name} must be a number, got {x!r}") from None


def check_nucleus_args(top_p, min_p):
    """the checks of generate()'s top_p / min_p, like check_sampling_args: plain Python, raised before anything touches a
    device.  Returns (top_p, min_p) as floats, None where left out."""
    if top_p is not None:
        p = _number(top_p, "top_p")
        if not (math.isfinite(p) and 0.0 < p <= 1.0):
            raise ValueError(f"generate: top_p must be in (0, 1] (or None), got {top_p!r}")
        top_p = p
    if min_p is not None:
        p = _number(min_p, "min_p")
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"generate: min_p must be in [0, 1] (or None), got {min_p!r}")
        min_p = p
    return top_p, min_p


def check_control_args(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, stop_tokens, pad_token, stop_poll,
                       vocab_size: int, ragged: bool = False):
    """the checks of generate()'s penalties, logit_bias and stop tokens, like check_nucleus_args: plain Python, raised before
    anything touches a device.  Returns None when every control is off, else a dict: rep / presence / frequency (floats), bias
    (a CPU fp32 tensor [V] or None), stop (a tuple of ints), pad (int), poll (int), adjust (bool: a penalty or a bias is on).
    ragged: the call has prompt_lengths -- it pads, so it needs a pad_token or stop_tokens, and always gets the dict."""
    V = int(vocab_size)

    def token(x, name):
        if isinstance(x, bool) or not isinstance(x, numbers.Integral):
            raise ValueError(f"generate: {name} must be an integer token id, got {x!r}")
        if not 0 <= int(x) < V:
            raise ValueError(f"generate: {name} must be in [0, {V}), got {x!r}")
        return int(x)

    rep = _number(repetition_penalty, "repetition_penalty")
    if not (math.isfinite(rep) and rep > 0.0):
        raise ValueError(f"generate: repetition_penalty must be finite and > 0, got {repetition_penalty!r}")
    presence = _number(presence_penalty, "presence_penalty")
    frequency = _number(frequency_penalty, "frequency_penalty")
    if not (math.isfinite(presence) and math.isfinite(frequency)):
        raise ValueError("generate: presence_penalty and frequency_penalty must be finite")
    if isinstance(stop_poll, bool) or not isinstance(stop_poll, numbers.Integral) or stop_poll < 1:
        raise ValueError(f"generate: stop_poll must be an integer >= 1, got {stop_poll!r}")
    bias = None
    if logit_bias is not None:
        if isinstance(logit_bias, dict):
            bias = torch.zeros(V, dtype=torch.float32)
            for k, v in logit_bias.items():
                bias[token(k, "a logit_bias token")] = _number(v, "a logit_bias value")
        else:
            try:
                bias = torch.as_tensor(logit_bias).detach().to(device="cpu", dtype=torch.float32)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError("generate: logit_bias must be a {token: value} dict or a sequence of vocab_size numbers") from None
            if bias.dim() != 1 or bias.numel() != V:
                raise ValueError(f"generate: a logit_bias sequence must have vocab_size = {V} entries, got {tuple(bias.shape)}")
            bias = bias.clone()
        if bool(torch.isnan(bias).any()) or bool((bias == math.inf).any()):
            raise ValueError("generate: logit_bias values must be finite or -inf (a ban)")
        if bool((bias == -math.inf).all()):
            raise ValueError("generate: logit_bias bans every token")
    stop = ()
    if stop_tokens is not None:
        if isinstance(stop_tokens, numbers.Integral) and not isinstance(stop_tokens, bool):
            seq = [stop_tokens]
        else:
            try:
                seq = list(stop_tokens)
            except TypeError:
                raise ValueError(f"generate: stop_tokens must be an int or a sequence of ints, got {stop_tokens!r}") from None
        stop = tuple(token(t, "a stop token") for t in seq)
        if not 1 <= len(stop) <= ops.SAMPLE_MAX_STOP or len(set(stop)) != len(stop):
            raise ValueError(f"generate: stop_tokens must be 1 to {ops.SAMPLE_MAX_STOP} distinct token ids, got {stop_tokens!r}")
    if pad_token is not None and not stop and not ragged:
        raise ValueError("generate: pad_token needs stop_tokens or prompt_lengths")
    if ragged and pad_token is None and not stop:
        raise ValueError("generate: prompt_lengths needs a pad_token (or stop_tokens, whose first one pads)")
    pad = token(pad_token, "pad_token") if pad_token is not None else (stop[0] if stop else 0)
    adjust = not (rep == 1.0 and presence == 0.0 and frequency == 0.0 and bias is None)       # do the logits change at all
    if not adjust and not stop and not ragged:
        return None
    return dict(rep=rep, presence=presence, frequency=frequency, bias=bias, stop=stop, pad=pad, poll=int(stop_poll), adjust=adjust)


def check_prompt_lengths(prompt_lengths, shape) -> Optional[tuple]:
    """the checks of generate()'s prompt_lengths, like check_control_args: plain Python, raised before anything touches a device
    (a tensor of lengths is read once, here).  B integers, a sequence or an integer tensor [B], with 1 <= p_b <= T for idx of
    `shape` (B, T).  Returns them as a tuple of ints; None when left out."""
    if prompt_lengths is None:
        return None
    if len(shape) != 2:
        raise ValueError("generate: prompt_lengths needs idx of shape (B, T)")
    B, T = int(shape[0]), int(shape[1])
    if isinstance(prompt_lengths, Tensor):
        if prompt_lengths.dim() != 1 or prompt_lengths.dtype == torch.bool or prompt_lengths.is_floating_point() \
                or prompt_lengths.is_complex():
            raise ValueError(f"generate: a prompt_lengths tensor must be [B] of an integer type, got {prompt_lengths.dtype} "
                             f"{tuple(prompt_lengths.shape)}")
        seq = prompt_lengths.tolist()
    else:
        try:
            seq = list(prompt_lengths)
        except TypeError:
            raise ValueError(f"generate: prompt_lengths must be a sequence or a tensor of B integers, got {prompt_lengths!r}") from None
    if len(seq) != B:
        raise ValueError(f"generate: prompt_lengths must have one entry per row of idx (B = {B}), got {len(seq)}")
    for p in seq:
        if isinstance(p, bool) or not isinstance(p, numbers.Integral):
            raise ValueError(f"generate: a prompt length must be an integer, got {p!r}")
        if not 1 <= int(p) <= T:
            raise ValueError(f"generate: a prompt length must be in [1, idx.shape[1] = {T}], got {p!r}")
    return tuple(int(p) for p in seq)


def stop_poll_due(poll: int, produced: int, lengths: Optional[Tensor]) -> bool:
    """the stop-poll rule of both device loops: every `poll` produced tokens (0: no stop tokens, never) one device-to-host read of
    lengths [B] -- has every row finished?"""
    return poll > 0 and produced % poll == 0 and bool((lengths != 0).all())


def trim_to_longest(ids: Tensor, lengths: Optional[Tensor], total: int, return_lengths: bool = False):
    """ids[:, :n], n = the longest row: a row's final length (stop token or the end of its budget included), `total` for a row
    still running.  lengths: the loop's int [B], 0 = running (None: every row ran to `total`).  return_lengths: (ids[:, :n], the
    rows' final lengths as int64 [B] on ids' device) -- what generate(return_lengths=True) returns."""
    n = None
    if lengths is not None:
        n = lengths.cpu()
        n = torch.where(n == 0, torch.full_like(n, total), n)
    out = ids[:, :total if n is None else int(n.max())]
    if not return_lengths:
        return out
    n = torch.full((ids.shape[0],), total) if n is None else n
    return out, n.to(device=ids.device, dtype=torch.int64)


class Generation(NamedTuple):
    """what generate(return_logprobs= / top_logprobs= / best_of=) returns.  ids (B, n) and lengths int64 [B]: what
    generate(return_lengths=True) returns.  logprobs fp32 (B, n), aligned with ids: the model's own log-probability
    (log_softmax of the raw logits: no temperature, penalty, bias or filter) of every token the row generated, its stop token
    included; 0.0 at prompt and padded positions, so logprobs.sum(1) is the log-likelihood of what the row generated.
    top_ids int32 / top_logprobs fp32 (B, n, top_logprobs): the most likely tokens at every generated position, descending,
    ties by lowest id; -1 / -inf at prompt and padded positions."""
    ids: Tensor
    lengths: Tensor
    logprobs: Tensor
    top_ids: Tensor
    top_logprobs: Tensor


class Score(NamedTuple):
    """what score() returns: per target position j (the token idx[:, j + 1] given idx[:, :j + 1]) logprobs fp32 (B, T - 1), ranks
    int32 (B, T - 1) (0: the model's greedy pick), top_ids int32 / top_logprobs fp32 (B, T - 1, top_logprobs), mask bool
    (B, T - 1).  Where mask is False (the target lies at or beyond the row's prompt_lengths entry) the four hold 0.0, -1, -1, -inf."""
    logprobs: Tensor
    ranks: Tensor
    top_ids: Tensor
    top_logprobs: Tensor
    mask: Tensor

    def perplexity(self) -> float:
        """exp(-mean log-probability) over the unmasked positions"""
        n = int(self.mask.sum())
        return math.exp(-float((self.logprobs.double() * self.mask).sum()) / n) if n else float("nan")

    def accuracy(self, k: int = 1) -> float:
        """the share of unmasked positions whose target is among the model's k most likely tokens"""
        n = int(self.mask.sum())
        return float(((self.ranks < k) & (self.ranks >= 0) & self.mask).sum()) / n if n else float("nan")


def check_logprob_args(return_logprobs, top_logprobs, best_of, has_pad: bool):
    """the checks of generate()'s return_logprobs / top_logprobs / best_of, like check_control_args: plain Python, raised before
    anything touches a device.  has_pad: the call has a pad_token or stop_tokens.  Returns (return_logprobs, top_logprobs, best_of)."""
    top = ops.check_top_logprobs(top_logprobs, "generate: top_logprobs")
    if isinstance(best_of, bool) or not isinstance(best_of, numbers.Integral) or best_of < 1:
        raise ValueError(f"generate: best_of must be an integer >= 1, got {best_of!r}")
    if best_of > 1 and not has_pad:
        raise ValueError("generate: best_of > 1 needs a pad_token (or stop_tokens, whose first one pads)")
    return bool(return_logprobs), top, int(best_of)


def new_score_buffers(B: int, n: int, device) -> tuple:
    """(logprobs fp32 (B, n) of 0.0, top_ids int32 (B, n, LOGPROBS_MAX_TOP) of -1, top_logprobs fp32 likewise of -inf): what a
    scored loop starts from -- dg_token_logprobs then writes the scored positions and nothing else"""
    return (torch.zeros((B, n), dtype=torch.float32, device=device),
            torch.full((B, n, ops.LOGPROBS_MAX_TOP), -1, dtype=torch.int32, device=device),
            torch.full((B, n, ops.LOGPROBS_MAX_TOP), -math.inf, dtype=torch.float32, device=device))


def make_generation(ids: Tensor, lengths: Optional[Tensor], total: int, logprobs: Tensor, top_ids: Tensor, top_logprobs: Tensor,
                    top_n: int) -> Generation:
    """the loops' full-width buffers (ids (B, >= total), logprobs (B, >= total), top_* (B, >= total, >= top_n)) trimmed to the
    longest row like trim_to_longest; lengths: the loop's int [B], 0 = running"""
    out, n = trim_to_longest(ids, lengths, total, True)
    w = out.shape[1]
    return Generation(out, n, logprobs[:, :w], top_ids[:, :w, :top_n], top_logprobs[:, :w, :top_n])


def select_best_of(logprobs: Tensor, lengths: Tensor, prompt_lengths, n: int) -> Tensor:
    """best_of's choice, on the B * n candidate rows (candidate c of prompt b is row b * n + c): per prompt the row with the highest
    mean log-probability over its generated tokens (positions [p, length), the stop token included; a row that generated nothing
    counts as -inf), ties to the lowest c.  Returns the B row indices (int64, CPU)."""
    lp = logprobs.detach().double().cpu()
    ln = lengths.detach().cpu().to(torch.int64)
    p = torch.as_tensor(prompt_lengths, dtype=torch.int64)
    count = (ln - p).clamp(min=0)
    mean = torch.where(count > 0, lp.sum(1) / count.clamp(min=1), torch.full_like(lp[:, 0], -math.inf)).view(-1, n)
    best = mean.max(dim=1, keepdim=True).values
    first = ((mean == best) | torch.isnan(mean)).to(torch.int64).argmax(dim=1)          # argmax of a 0/1 row: its first 1
    return torch.arange(mean.shape[0]) * n + first


def keep_best_of(gen: Generation, prompt_lengths, n: int, pad: int) -> Generation:
    """the B kept rows of a B * n-row Generation, trimmed again to the longest of them"""
    rows = select_best_of(gen.logprobs, gen.lengths, prompt_lengths, n).to(gen.ids.device)
    w = max(int(gen.lengths[rows].max()), 1)
    return Generation(gen.ids[rows, :w], gen.lengths[rows], gen.logprobs[rows, :w], gen.top_ids[rows, :w], gen.top_logprobs[rows, :w])


class ControlOperands:
    """what a generate() call with controls hands to ops.sample_rows (dg_sample_rows_control): the 16-word control block, bias [V],
    the token counts [B, V] of the whole sequence so far (prompt included, beyond the context window too; the kernel adds the token
    it writes) and lengths [B], the rows' "finished" state under the device sampler's stop tokens.  The eager loops allocate one
    per call (fresh); a DeviceDecoder keeps one for good, since its graphs hold the addresses.  begin() starts a call on either.
    spans [B, 2]: the rows' {prompt length, prompt length + budget} of a call with prompt_lengths (dg_sample_rows_ragged)."""

    def __init__(self, B: int, V: int, device, bias: bool = True, lengths: bool = True, spans: bool = False):
        self.control = ops.new_sample_control(device=device)          # controls off: what a capture's warm-up may safely run on
        self.bias = torch.zeros(V, dtype=torch.float32, device=device) if bias else None
        self.counts = torch.zeros((B, V), dtype=torch.int32, device=device)
        self.lengths = torch.zeros(B, dtype=torch.int32, device=device) if lengths else None
        self.spans = torch.zeros((B, 2), dtype=torch.int32, device=device) if spans else None

    @classmethod
    def fresh(cls, ctl: Optional[dict], idx: Tensor, V: int, lengths: bool, first: Optional[tuple] = None,
              n_new: int = 0) -> Optional["ControlOperands"]:
        """an eager call's own operands, begun on the prompt idx (None without controls): a bias, lengths and spans only where it
        has them (first: the checked prompt_lengths, whose budget ends a row as a stop token does)"""
        if ctl is None:
            return None
        cs = cls(idx.shape[0], V, idx.device, bias=ctl["bias"] is not None, lengths=lengths and (bool(ctl["stop"]) or first is not None),
                 spans=first is not None)
        cs.begin(ctl, idx, idx.shape[1], first, n_new)
        return cs

    @torch.no_grad()
    def begin(self, ctl: dict, ids: Tensor, t0: int, first: Optional[tuple] = None, n_new: int = 0) -> None:
        """the start of a call: the block of check_control_args' dict, its bias (None: zeros, and the block's use_bias is 0), the
        counts of the prompt ids[:, :t0] and all rows running -- nothing is inherited from an earlier call.  first (the checked
        prompt_lengths): spans = {p_b, p_b + n_new}, and row b's counts are those of its own prompt ids[b, :p_b], the whole of it --
        a row's counts are first read when it first samples, and by then its sequence holds all of its prompt"""
        self.control.copy_(ops.new_sample_control(
            repetition_penalty=ctl["rep"], presence_penalty=ctl["presence"], frequency_penalty=ctl["frequency"], stop_tokens=ctl["stop"],
            pad_token=ctl["pad"], use_bias=ctl["bias"] is not None, device=self.control.device))
        if self.bias is not None:
            if ctl["bias"] is None:
                self.bias.zero_()
            else:
                self.bias.copy_(ctl["bias"])
        if first is None:
            ops.token_counts(ids, t0, self.counts.shape[1], self.counts)
        else:
            self.spans.copy_(torch.tensor([[p, p + n_new] for p in first], dtype=torch.int32))
            ops.token_counts(ids, self.spans[:, 0], self.counts.shape[1], self.counts)
        if self.lengths is not None:
            self.lengths.zero_()

    def kw(self, ragged: bool = False) -> dict:
        """ops.sample_rows' keywords; ragged: with the spans, and so dg_sample_rows_ragged"""
        kw = dict(control=self.control, bias=self.bias, counts=self.counts, lengths=self.lengths)
        return dict(kw, spans=self.spans) if ragged else kw


def draw_seed(generator: Optional[torch.Generator]) -> int:
    """one sampling seed from the CPU generator (the global one unless `generator` is given)"""
    return int(torch.randint(0, 2 ** 62, (1,), generator=generator))


class Sampling(NamedTuple):
    """one checked generate() request: what travels from generate() to the token loops.  Sampling.checked builds it from
    generate()'s arguments; ctl is check_control_args' dict (None: every control off)."""
    sampler: str = "host"
    temperature: float = 1.0
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    min_p: Optional[float] = None
    ctl: Optional[dict] = None
    generator: Optional[torch.Generator] = None
    seed: Optional[int] = None
    prompt_lengths: Optional[tuple] = None          # check_prompt_lengths' tuple: the rows' own prompt lengths in a right-padded idx
    return_lengths: bool = False
    logprobs: bool = False                          # return_logprobs
    top_logprobs: int = 0
    best_of: int = 1

    @classmethod
    def checked(cls, vocab_size: int, generator, sampler, temperature, top_k, seed, top_p, min_p, repetition_penalty, presence_penalty,
                frequency_penalty, logit_bias, stop_tokens, pad_token, stop_poll, prompt_lengths=None, shape=(),
                return_lengths: bool = False, return_logprobs: bool = False, top_logprobs: int = 0, best_of: int = 1) -> "Sampling":
        """the argument checks of generate(), all of them: plain Python, raised before anything touches a device (shape: idx's,
        which prompt_lengths is checked against)"""
        temperature, top_k = check_sampling_args(sampler, temperature, top_k, vocab_size)
        top_p, min_p = check_nucleus_args(top_p, min_p)
        prompt_lengths = check_prompt_lengths(prompt_lengths, shape)
        logprobs, top_logprobs, best_of = check_logprob_args(return_logprobs, top_logprobs, best_of,
                                                             pad_token is not None or stop_tokens is not None)
        # best_of pads like a ragged call does (its candidates end at different lengths): it always gets the dict
        ctl = check_control_args(repetition_penalty, presence_penalty, frequency_penalty, logit_bias, stop_tokens, pad_token,
                                 stop_poll, vocab_size, ragged=prompt_lengths is not None or best_of > 1)
        if best_of > 1 and prompt_lengths is not None:
            prompt_lengths = tuple(p for p in prompt_lengths for _ in range(best_of))          # candidate c of prompt b: row b * n + c
        return cls(sampler, temperature, top_k, top_p, min_p, ctl, generator, seed, prompt_lengths, bool(return_lengths), logprobs,
                   top_logprobs, best_of)

    @property
    def scored(self) -> bool:
        """the call asks for log-probabilities (return_logprobs, top_logprobs or best_of): it returns a Generation"""
        return self.logprobs or self.top_logprobs > 0 or self.best_of > 1

    def deliver(self, gen: "Generation", T: int) -> "Generation":
        """a scored call's result: with best_of the kept row of every prompt (T: idx.shape[1], the prompt length without
        prompt_lengths)"""
        if self.best_of == 1:
            return gen
        first = self.prompt_lengths if self.prompt_lengths is not None else (T,) * gen.ids.shape[0]
        return keep_best_of(gen, first, self.best_of, self.ctl["pad"])

    @property
    def ragged(self) -> bool:
        """the call has prompt_lengths: one shared position walks rows that start at different lengths"""
        return self.prompt_lengths is not None

    def span(self, T: int, n_new: int) -> tuple:
        """(the loops' first position, their last + 1) for idx (B, T): (T, T + n_new), or with prompt_lengths
        (min p_b, max p_b + n_new)"""
        if self.prompt_lengths is None:
            return T, T + n_new
        return min(self.prompt_lengths), max(self.prompt_lengths) + n_new

    def enter(self, idx: Tensor, n_new: int):
        """prompt_lengths only (else (idx, None)): idx cropped to the longest prompt with pad_token at and beyond every row's own
        length -- whatever the caller's padding holds never reaches a kernel, the id range check or the result -- and, for a call
        that asks for no new token, its result"""
        if self.best_of > 1:
            idx = idx.repeat_interleave(self.best_of, dim=0)
        if self.prompt_lengths is None:
            return idx, None
        p = torch.tensor(self.prompt_lengths, device=idx.device)
        idx = idx[:, :max(self.prompt_lengths)]
        keep = torch.arange(idx.shape[1], device=idx.device)[None, :] < p[:, None]
        idx = torch.where(keep, idx, torch.full_like(idx, self.ctl["pad"]))
        if n_new >= 1:
            return idx, None
        if self.scored:
            return idx, self.deliver(make_generation(idx, p, idx.shape[1], *new_score_buffers(idx.shape[0], idx.shape[1], idx.device),
                                                     self.top_logprobs), idx.shape[1])
        return idx, trim_to_longest(idx, p, idx.shape[1], self.return_lengths)

    @property
    def adjust(self) -> bool:
        """a penalty or a bias is on: the logits change (stop tokens alone change no distribution)"""
        return self.ctl is not None and self.ctl["adjust"]

    @property
    def stop(self) -> tuple:
        return () if self.ctl is None else self.ctl["stop"]

    @property
    def poll(self) -> int:
        """the device loops' stop_poll; 0 without stop tokens"""
        return self.ctl["poll"] if self.stop else 0

    def params(self, device, graph: bool = False) -> Optional[Tensor]:
        """the parameter block of this request, and with it the kernel entry.  None: the plain softmax, the reference's distribution.
        Four words {inv_temp, top_k, top_p, min_p} where dg_sample_rows_control runs (host: a penalty or a bias; device: any control,
        a stop token alone included), for a DeviceDecoder's steps (graph: one capture serves every setting) and with a top_p or a
        min_p; two words {inv_temp, top_k} otherwise."""
        four = graph or (self.adjust if self.sampler == "host" else self.ctl is not None)
        if self.sampler == "host" and not four and (self.temperature, self.top_k, self.top_p, self.min_p) == (1.0, None, None, None):
            return None
        return ops.new_sample_params(self.temperature, self.top_k, device, top_p=self.top_p, min_p=self.min_p, four=four)

    def first_state(self, device, t0: int) -> Tensor:
        """the device sampler's decode state at sequence length t0; the seed is drawn here, once, from the CPU generator if not given"""
        seed = draw_seed(self.generator) if self.seed is None else self.seed
        return ops.new_rng_state(int(seed), device, step=t0)


class _LM(HipModule):
    """forward/generate scaffolding shared by the five position-aware models."""

    context_length: Optional[int]

    def _embed(self, idx):
        return HF.embed(idx, self.token_embedding_table.weight, self.position_embedding_table.weight)

    def _body(self, x, rng):          # overridden
        raise NotImplementedError

    def _any_dropout(self) -> bool:
        return False

    def _head(self, x):
        return HF.linear(x, self.lm_head.weight, self.lm_head.bias, "bf16x3" if self.split_bf16 else self.act_dtype)

    check_ids = True      # False: skip the id range check (one or two device-to-host syncs per forward that nn.Embedding does not
                          # have) once a data source has been validated -- ids out of range are then CLAMPED by the kernels

    def _check_ids(self, idx, targets):
        ops._chk(idx, "idx", torch.int64, contiguous=False)
        if targets is not None:
            ops._chk(targets, "targets", torch.int64, contiguous=False)
        if not self.check_ids:
            return
        V = self.token_embedding_table.weight.shape[0]
        ops.check_ids(idx, V, "idx")
        if targets is not None:
            ops.check_ids(targets, V if not hasattr(self, "lm_head") else self.lm_head.weight.shape[0], "targets", allow=self.ignore_index)

    # the training objective's options: plain attributes, not part of the state_dict; forward applies them in train() mode only
    label_smoothing = 0.0
    z_loss = 0.0
    ignore_index = None

    def set_loss_options(self, label_smoothing=0.0, z_loss=0.0, ignore_index=None):
        """label smoothing (F.cross_entropy's label_smoothing) and the z-loss coefficient (z_loss * logsumexp^2 per row) of
        the loss forward(idx, targets) returns in train() mode; in eval() it stays the plain cross entropy, the reference's metric.
        ignore_index (F.cross_entropy's ignore_index; None: off, -100: the reference's behaviour) describes the targets, not the
        objective: a target equal to it is left out of the mean, in train() and in eval()."""
        self.label_smoothing, self.z_loss, self.ignore_index = ops.check_loss_options(label_smoothing, z_loss, ignore_index)
        return self

    # document mask: like ignore_index it describes the data, not the objective -- a plain attribute, applied in train() and eval()
    doc_separator = None

    def set_doc_separator(self, token_id=None):
        """token_id (None: off): a document of the packed batch ends WITH this token, and forward(idx, targets) lets no token
        attend across it -- query t sees the keys from 1 + the last separator before t (dg_doc_starts, the DOC attention
        kernels), in train() and in eval().  Position embeddings are not reset per document.  generate does not apply the mask."""
        if token_id is not None:
            V = self.token_embedding_table.weight.shape[0]
            if isinstance(token_id, bool) or not isinstance(token_id, int) or not 0 <= token_id < V:
                raise ValueError(f"doc separator {token_id!r} is not a token id in [0, {V})")
        self.doc_separator = token_id
        return self

    def _set_doc_starts(self, starts):
        from .model_component import Head, _MultiHeadBase
        for m in self.modules():
            if isinstance(m, (Head, _MultiHeadBase)):
                m._doc_starts = starts

    def _unmasked(self, idx):
        """forward(idx) without the document mask: generate's logits source"""
        sep = self.doc_separator
        if sep is None:
            return self(idx)
        self.doc_separator = None
        try:
            return self(idx)
        finally:
            self.doc_separator = sep

    def _loss(self, logits, targets):
        if self.training:
            return HF.cross_entropy(logits, targets, self.label_smoothing, self.z_loss, self.ignore_index)
        return HF.cross_entropy(logits, targets, ignore_index=self.ignore_index)

    def forward(self, idx, targets=None):
        if idx.dim() != 2:
            raise ValueError("idx must be (B, T)")
        self._check_ids(idx, targets)
        rng = self._rng_snapshot(idx.device, self._any_dropout())
        if self.doc_separator is None:
            logits = self._head(self._body(self._embed(idx), rng))
        else:
            self._set_doc_starts(ops.doc_starts(idx if idx.stride(1) == 1 else idx.contiguous(), self.doc_separator))
            try:
                logits = self._head(self._body(self._embed(idx), rng))
            finally:
                self._set_doc_starts(None)
        if targets is None:
            return logits, None
        B, T, V = logits.shape
        logits = logits.view(B * T, V)
        loss = self._loss(logits, targets.reshape(B * T))
        return logits, loss

    def _window_logits(self, idx):
        """the host loop's logits source of every model: the full forward on the cropped window, last position"""
        cond = idx if self.context_length is None else idx[:, -self.context_length:]
        logits, _ = self._unmasked(cond.contiguous())
        return logits[:, -1, :]

    @staticmethod
    def _probs(logits, params, cs=None):
        """params None: the plain softmax (the reference's distribution); else the temperature / top-k / top-p / min-p filtered one;
        with cs (ControlOperands, given when a penalty or a bias is on) the same kernel applies those too and only reads the counts.
        Stop tokens alone change no distribution: the call a run without them makes, so the tokens before a stop are its tokens"""
        if cs is None and params is None:
            return ops.softmax_rows(logits)
        return ops.sample_rows(logits, params=params, tokens=False, probs=True, **({} if cs is None else cs.kw()))

    def generate(self, idx, max_new_tokens, generator: Optional[torch.Generator] = None, *, sampler: str = "host",
                 temperature: float = 1.0, top_k: Optional[int] = None, seed: Optional[int] = None,
                 top_p: Optional[float] = None, min_p: Optional[float] = None, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias=None, stop_tokens=None,
                 pad_token: Optional[int] = None, stop_poll: int = 64, prompt_lengths=None, return_lengths: bool = False,
                 return_logprobs: bool = False, top_logprobs: int = 0, best_of: int = 1):
        """ref: src/model.py:611-636.  sampler="host" (default): softmax runs on the GPU; torch.multinomial runs on the host CPU
        generator (the global one unless `generator` is given), as it does in the reference on CPU.  A temperature other than 1
        (0 = greedy) or a top_k filters the distribution on the GPU first (dg_sample_rows); so do top_p (nucleus: the most
        likely tokens whose mass reaches top_p, ties kept) and min_p (tokens at least min_p times as likely as the best one),
        applied after top_k (dg_sample_rows_nucleus).
        sampler="device": the tokens are drawn by dg_sample_rows from a counter-based stream keyed by `seed` (drawn once from the
        CPU generator when None) and the sequence length, and never leave the GPU inside the loop.
        Controls, all off by default, applied to the logits before the temperature (dg_sample_rows_control):
        repetition_penalty (CTRL / HF: a seen token's logit is divided by it when positive, multiplied when not),
        presence_penalty (subtracted once from a seen token) and frequency_penalty (subtracted per occurrence) act on the token
        counts of the WHOLE sequence so far -- the prompt included, also what has left the context window, as HF's processors
        see input_ids.  logit_bias: a {token: value} dict or vocab_size values added to the logits; -inf bans a token.
        stop_tokens (an int or up to 8): a row that draws one keeps it, every later position of that row is pad_token (default: the
        first stop token), and the result (B, t0 + n), n <= max_new_tokens, is trimmed to the longest row; before its stop a row
        has the tokens of the same call without stop_tokens.  With the device sampler the host looks at the rows' state every
        stop_poll tokens (the only sync; the result does not depend on it).
        prompt_lengths (B integers, 1 <= p_b <= idx.shape[1]): the rows of idx are prompts of different lengths, right-padded;
        what idx holds at or beyond column p_b is replaced by pad_token on entry and read by nothing.  It needs a pad_token or
        stop_tokens.  Every row gets up to max_new_tokens tokens after its own prompt: the result (B, n), n = the longest final
        row, holds per row the prompt, its tokens, then pad_token; a row ends at p_b + max_new_tokens or at its stop token.  One
        shared position walks all rows from min p_b: a row still inside its prompt keeps its prompt token, a row past it samples
        (dg_sample_rows_ragged), so row b has the tokens of a call on prompt b alone in that row with the same seed.
        return_lengths=True: (ids, the rows' final lengths as int64 [B]), in any call.
        return_logprobs=True, top_logprobs=n (0..20) or best_of=n: the call returns a Generation (see there) -- per generated token
        the model's own log-probability (log_softmax of the raw logits, dg_token_logprobs: no temperature, penalty, bias or filter;
        the stop token's own position included, 0.0 at prompt and padded positions) and the top_logprobs most likely tokens; one
        more launch per token, and the tokens are bit for bit those of the call without them.  best_of=n draws n candidates per
        prompt (row b * n + c) and keeps the one with the highest mean log-probability over its generated tokens, ties to the
        lowest c; it pads, so it needs a pad_token or stop_tokens.  The numbers equal score() of the returned text.
        The document mask (set_doc_separator) is NOT applied here: the tokens with a separator set are bit for bit those without.
        To end a sample at the end of its document, pass stop_tokens=[sep]."""
        req = Sampling.checked(self.token_embedding_table.weight.shape[0], generator, sampler, temperature, top_k, seed, top_p, min_p,
                               repetition_penalty, presence_penalty, frequency_penalty, logit_bias, stop_tokens, pad_token, stop_poll,
                               prompt_lengths, tuple(getattr(idx, "shape", ())), return_lengths, return_logprobs, top_logprobs, best_of)
        T = idx.shape[1] if getattr(idx, "dim", lambda: 0)() == 2 else 0
        idx, done = req.enter(idx, max_new_tokens)
        if done is not None:
            return done
        out = (self._generate_device if sampler == "device" else self._generate_host)(idx, max_new_tokens, req)
        return req.deliver(out, T) if req.scored else out

    @torch.no_grad()
    def score(self, idx, prompt_lengths=None, top_logprobs: int = 0) -> Score:
        """the model's log-probability of every token of idx (B, T) given the tokens before it: per-token log-likelihood,
        perplexity, accuracy@k.  One forward pass in eval() semantics (no dropout, whatever mode the model is in; like generate,
        without the document mask) on idx[:, :-1], then ONE dg_token_logprobs launch over its B * (T - 1) rows of logits, read in
        the dtype the forward wrote them in, with the targets idx[:, 1:] -- no (B * T, V) log-softmax exists at any point.
        prompt_lengths (B integers, 1 <= p_b <= T): row b holds p_b tokens, right-padded; what lies beyond is read by nothing and
        the positions whose target lies there are masked.  top_logprobs in [0, 20]: also the most likely tokens per position.
        The numbers are those generate(return_logprobs=True) reports for the same tokens.  T - 1 must fit the context window."""
        top_n = ops.check_top_logprobs(top_logprobs, "score: top_logprobs")
        first = check_prompt_lengths(prompt_lengths, tuple(getattr(idx, "shape", ())))
        ops._chk(idx, "idx", torch.int64, contiguous=False)
        if idx.dim() != 2 or idx.shape[1] < 2:
            raise ValueError("score: idx must be (B, T) with T >= 2")
        B, T = idx.shape
        pos = torch.arange(1, T, device=idx.device)[None, :]                      # the targets' positions
        mask = (pos < torch.tensor(first, device=idx.device)[:, None]) if first is not None else torch.ones((B, T - 1), dtype=torch.bool, device=idx.device)
        if first is not None:                                                      # the padding never reaches a kernel or the id check
            idx = idx.clone()
            idx[:, 1:][~mask] = 0
        was = self.training
        self.eval()
        try:
            logits, _ = self._unmasked(idx[:, :-1].contiguous())
        finally:
            self.train(was)
        V = logits.shape[-1]
        res = ops.token_logprobs(logits.view(B * (T - 1), V), idx[:, 1:].reshape(-1), top_n=top_n, rank=True)
        lp, rk = res[0].view(B, T - 1), res[1].view(B, T - 1)
        ti = res[2].view(B, T - 1, top_n) if top_n else torch.empty((B, T - 1, 0), dtype=torch.int32, device=idx.device)
        tl = res[3].view(B, T - 1, top_n) if top_n else torch.empty((B, T - 1, 0), dtype=torch.float32, device=idx.device)
        if first is not None:
            lp = torch.where(mask, lp, torch.zeros_like(lp))
            rk = torch.where(mask, rk, torch.full_like(rk, -1))
            ti = torch.where(mask[:, :, None], ti, torch.full_like(ti, -1))
            tl = torch.where(mask[:, :, None], tl, torch.full_like(tl, -math.inf))
        return Score(lp, rk, ti, tl, mask)

    @torch.no_grad()
    def _generate_host(self, idx, max_new_tokens, req: Sampling, source=None):
        """the host loop, the reference's: per token the last-position logits of the sequence so far from `source` (default: the
        full forward on the cropped window), their distribution, ONE multinomial on the CPU generator, the stop rule, append,
        count.  Stop rule: a finished row gets pad_token; a row that draws a stop token keeps it and is finished from the next
        position on; the loop ends once every row is.  With prompt_lengths the loop starts from idx[:, :min p_b]; a row still
        inside its prompt takes its prompt token in the place of its draw (forced: already in its counts, and never a stop), and
        a row that receives the last token of its budget is finished under the same rule."""
        V = self.token_embedding_table.weight.shape[0]
        source = source or self._window_logits
        params = req.params(idx.device)
        cs = ControlOperands.fresh(req.ctl, idx, V, lengths=False, first=req.prompt_lengths, n_new=max_new_tokens)
        t0, total = req.span(idx.shape[1], max_new_tokens)
        finished = torch.zeros(idx.shape[0], dtype=torch.bool)
        ends = req.stop or req.ragged                    # rows can end before the loop does
        final = torch.zeros(idx.shape[0], dtype=torch.int64) if ends else None          # 0: running
        if req.ragged:
            prompt, first = idx.cpu(), torch.tensor(req.prompt_lengths)
            idx = idx[:, :t0]
        scores = new_score_buffers(idx.shape[0], total, idx.device) if req.scored else None
        for L in range(t0, total):
            logits = source(idx)
            probs = self._probs(logits, params, cs if req.adjust else None)
            unscored = finished                      # the rows that were finished before this position, or are forced at it
            nxt = torch.multinomial(probs.cpu(), num_samples=1, generator=req.generator)
            forced = None
            if req.ragged and L < prompt.shape[1]:
                forced = first > L
                nxt = torch.where(forced[:, None], prompt[:, L:L + 1], nxt)
            if ends:
                nxt = torch.where(finished[:, None], torch.full_like(nxt, req.ctl["pad"]), nxt)
                hit = torch.isin(nxt[:, 0], torch.tensor(req.stop)) if req.stop else torch.zeros_like(finished)
                if req.ragged:
                    hit = (hit if forced is None else hit & ~forced) | (first + max_new_tokens <= L + 1)
                final = torch.where(hit & ~finished, torch.full_like(final, L + 1), final)
                finished = finished | hit
            nxt = nxt.to(idx.device)
            idx = torch.cat((idx, nxt), dim=1)
            if scores is not None:                   # one dg_token_logprobs launch after the token is placed
                res = ops.token_logprobs(logits, nxt[:, 0].contiguous(), top_n=req.top_logprobs)
                keep = ~(unscored if forced is None else unscored | forced).to(idx.device)
                lp, top = (res[0], res[1:]) if req.top_logprobs else (res, ())
                scores[0][:, L] = torch.where(keep, lp, torch.zeros_like(lp))
                for buf, t in zip(scores[1:], top):
                    buf[:, L, :req.top_logprobs] = torch.where(keep[:, None], t, buf[:, L, :req.top_logprobs])
            if req.adjust:
                ops.token_counts(nxt, 1 if forced is None else (~forced).to(device=idx.device, dtype=torch.int32), V, cs.counts,
                                 accumulate=True)
            if ends and bool(finished.all()):
                break
        if scores is not None:
            return make_generation(idx, final, total, *scores, req.top_logprobs)
        return trim_to_longest(idx, final, total, req.return_lengths)

    @staticmethod
    def _prompt_shape(idx):          # the device-sampler paths' first check
        ops._chk(idx, "idx", torch.int64, contiguous=False)
        if idx.dim() != 2 or idx.shape[1] < 1:
            raise ValueError("idx must be (B, T) with T >= 1")
        return idx.shape

    def _decode_begin(self, idx, req: Sampling, ids, t0: int, graph: bool = False):
        """the device-sampler paths' start: the prompt is range-checked once and goes into ids; returns (decode state at the first
        position t0, params)"""
        self._check_ids(idx, None)
        ids[:, :idx.shape[1]] = idx
        return req.first_state(idx.device, t0), req.params(idx.device, graph)

    @torch.no_grad()
    def _generate_device(self, idx, max_new_tokens, req: Sampling):
        """the reference algorithm (full forward on the cropped window per token) with the sampler on the device: the kernel writes
        token L into ids[:, L]; no host copy or sync inside the loop (the ids were range-checked once, sampled ids are in range).
        With stop tokens the host reads the rows' lengths every req.poll tokens and leaves once every row is finished.
        With prompt_lengths L starts at min p_b and every step ends in dg_sample_rows_ragged, which leaves the rows still inside
        their prompts alone."""
        B, T = self._prompt_shape(idx)
        (t0, total), ctx = req.span(T, max_new_tokens), self.context_length
        ids = torch.zeros((B, total), dtype=torch.int64, device=idx.device)
        state, params = self._decode_begin(idx, req, ids, t0)
        cs = ControlOperands.fresh(req.ctl, idx, self.token_embedding_table.weight.shape[0], lengths=True, first=req.prompt_lengths,
                                   n_new=max_new_tokens)
        kw = {} if cs is None else cs.kw(req.ragged)
        lengths = cs.lengths if req.poll or req.ragged else None
        scores = new_score_buffers(B, total, idx.device) if req.scored else None
        skw = None if scores is None else dict(
            state=state, lengths=None if cs is None else cs.lengths, spans=cs.spans if req.ragged else None, out=scores[0],
            out_top_ids=scores[1], out_top_lp=scores[2], top_n=torch.tensor([req.top_logprobs], dtype=torch.int32, device=idx.device))
        saved = self.__dict__.get("check_ids")           # None: the class's default is in force
        self.check_ids = False
        try:
            for L in range(t0, total):
                lo = 0 if ctx is None else max(0, L - ctx)
                logits, _ = self._unmasked(ids[:, lo:L].contiguous())
                ops.sample_rows(logits[:, -1, :], state, params, ids=ids, **kw)
                if skw is not None:                  # one launch after the token is placed, before the position moves on
                    ops.token_logprobs(logits[:, -1, :], ids, **skw)
                ops.state_advance(state)
                if stop_poll_due(req.poll, L + 1 - t0, lengths):
                    break
        finally:
            del self.check_ids
            if saved is not None:
                self.check_ids = saved
        if scores is not None:
            return make_generation(ids, lengths, total, *scores, req.top_logprobs)
        return trim_to_longest(ids, lengths, total, req.return_lengths)


class BigramLM(_LM):
    """ref: src/model.py:65-130: logits are a (V,V) table lookup."""

    def __init__(self, vocab_size, *, precision: str = "fp32"):
        super().__init__(precision)
        self.context_length = None
        self.token_embedding_table = nn.Embedding(vocab_size, vocab_size)

    def forward(self, idx, targets=None):
        self._check_ids(idx, targets)
        logits = HF.embed(idx, self.token_embedding_table.weight, None)
        if targets is None:
            return logits, None
        B, T, V = logits.shape
        logits = logits.view(B * T, V)
        return logits, self._loss(logits, targets.reshape(B * T))


class SingleHeadAttentionLM(_LM):
    """ref: src/model.py:133-227."""

    def __init__(self, vocab_size, embedding_dim, context_length, head_size, *, precision: str = "fp32"):
        super().__init__(precision)
        self.context_length = context_length
        self.token_embedding_table = nn.Embedding(vocab_size, embedding_dim)
        self.position_embedding_table = nn.Embedding(context_length, embedding_dim)
        self.sa_head = Head(head_size, embedding_dim, context_length, precision=precision)
        self.lm_head = nn.Linear(embedding_dim, vocab_size)

    def _body(self, x, rng):
        return self.sa_head(x)


class MultiHeadAttentionLM(_LM):
    """ref: src/model.py:230-331."""

    def __init__(self, vocab_size, embedding_dim, context_length, head_size, num_heads, *, precision: str = "fp32"):
        super().__init__(precision)
        self.context_length = context_length
        self.token_embedding_table = nn.Embedding(vocab_size, embedding_dim)
        self.position_embedding_table = nn.Embedding(context_length, embedding_dim)
        self.sa_head = MultiHeadAttention(num_heads, head_size // num_heads, embedding_dim, context_length, precision=precision)
        self.lm_head = nn.Linear(embedding_dim, vocab_size)

    def _body(self, x, rng):
        return self.sa_head(x)


class _BlocksLM(_LM):
    def _body(self, x, rng):
        for blk in self.blocks:
            x = blk(x, rng)
        return x


class BlocksLM(_BlocksLM):
    """ref: src/model.py:334-432."""

    def __init__(self, vocab_size, embedding_dim, context_length, num_heads, num_layers, *, precision: str = "fp32"):
        super().__init__(precision)
        self.context_length = context_length
        self.token_embedding_table = nn.Embedding(vocab_size, embedding_dim)
        self.position_embedding_table = nn.Embedding(context_length, embedding_dim)
        self.blocks = nn.Sequential(*[Block(embedding_dim, context_length, num_heads, precision=precision) for _ in range(num_layers)])
        self.lm_head = nn.Linear(embedding_dim, vocab_size)


class ResidualBlocksLM(_BlocksLM):
    """ref: src/model.py:435-533."""

    def __init__(self, vocab_size, embedding_dim, context_length, num_heads, num_layers, *, precision: str = "fp32"):
        super().__init__(precision)
        self.context_length = context_length
        self.token_embedding_table = nn.Embedding(vocab_size, embedding_dim)
        self.position_embedding_table = nn.Embedding(context_length, embedding_dim)
        self.blocks = nn.Sequential(*[ResidualBlock(embedding_dim, num_heads, context_length, precision=precision) for _ in range(num_layers)])
        self.lm_head = nn.Linear(embedding_dim, vocab_size)


class TransformerLM(_BlocksLM):
    """ref: src/model.py:535-636."""

    def __init__(self, vocab_size, embedding_dim, context_length, num_heads, num_layers, dropout, *, precision: str = "fp32"):
        super().__init__(precision)
        self.context_length = context_length
        self.token_embedding_table = nn.Embedding(vocab_size, embedding_dim)
        self.position_embedding_table = nn.Embedding(context_length, embedding_dim)
        self.blocks = nn.Sequential(
            *[ResidualBlock2(embedding_dim, num_heads, context_length, dropout, precision=precision) for _ in range(num_layers)])
        for l, blk in enumerate(self.blocks):
            blk.set_layer_index(l)
        self.ln_f = nn.LayerNorm(embedding_dim)      # never applied: src/model.py:598-599
        self.lm_head = nn.Linear(embedding_dim, vocab_size)
        self._p = float(dropout)

    def _any_dropout(self) -> bool:
        return self._p > 0.0


    # ------------------------------------------------------------------ KV-cached decoding
    @torch.no_grad()
    def _decode_weights(self):
        from . import sublayers as S
        wp = S.OnTheFlyWeights(self.act_dtype)
        ws = []
        for blk in self.blocks:
            heads = list(blk.sa_head.heads)
            wqkv = torch.cat([h.query.weight for h in heads] + [h.key.weight for h in heads] + [h.value.weight for h in heads], 0)
            ws.append(dict(ln1w=blk.ln1.weight, ln1b=blk.ln1.bias, wqkv=wp.fwd(wqkv), wproj=wp.fwd(blk.sa_head.proj.weight),
                           bproj=blk.sa_head.proj.bias, ln2w=blk.ln2.weight, ln2b=blk.ln2.bias, w1=wp.fwd(blk.ffwd.net[0].weight),
                           b1=blk.ffwd.net[0].bias, w2=wp.fwd(blk.ffwd.net[2].weight), b2=blk.ffwd.net[2].bias))
        return ws, wp.fwd(self.lm_head.weight)

    def _heads(self):
        """(number of heads, head size)"""
        heads = self.blocks[0].sa_head.heads
        return len(heads), heads[0].head_size

    def _layers(self, x, ws, attend):
        """the layer stack on the fp32 rows x, written once: per layer LN, attend(l, h, wqkv) -- the QKV GEMM and the attention of
        the caller's kind, on the normalised rows h -- proj + residual, LN, FFN + residual"""
        act, sp = self.act_dtype, self.split_bf16          # precision bf16x3: split-bf16 contractions
        for l, W in enumerate(ws):
            h, _, _ = ops.layernorm_fwd(x, W["ln1w"], W["ln1b"], act)
            o = attend(l, h, W["wqkv"])
            x = ops.gemm_nt(o, W["wproj"], torch.float32, bias=W["bproj"], residual=x, split=sp)
            h, _, _ = ops.layernorm_fwd(x, W["ln2w"], W["ln2b"], act)
            f = ops.gemm_nt(h, W["w1"], act, bias=W["b1"], relu=True, split=sp)
            x = ops.gemm_nt(f, W["w2"], torch.float32, bias=W["b2"], residual=x, split=sp)
        return x

    def _lm_logits(self, x, w_lm, lm_bias=None):
        """the cast and lm_head on the rows x (B, C) -> fp32 logits (B, V); lm_bias: a staged copy to use in place of lm_head.bias"""
        xa = x if self.act_dtype == torch.float32 else ops.cast(x, self.act_dtype)
        return ops.gemm_nt(xa, w_lm, torch.float32, bias=self.lm_head.bias if lm_bias is None else lm_bias, split=self.split_bf16)

    @torch.no_grad()
    def _decode_step(self, tok_col, t, caches, ws, w_lm):
        """logits (B, V) of the token at position t; K/V of position t are appended to the caches."""
        NH, H = self._heads()

        def attend(l, h, wqkv):
            ops.gemm_nt(h, wqkv, self.act_dtype, out=caches[l][:, t], split=self.split_bf16)      # q/k/v row t straight into the cache
            return ops.attn_decode(caches[l], t, NH, H, H ** -0.5)

        B = tok_col.shape[0]
        x = ops.embed_fwd(tok_col, self.token_embedding_table.weight, self.position_embedding_table.weight[t:t + 1]).view(B, -1)
        return self._lm_logits(self._layers(x, ws, attend), w_lm)

    @torch.no_grad()
    def _forward_rows(self, x, B, T, caches, ws, w_lm, lm_bias=None):
        """x (B*T, C), the embedded rows of B sequences of T positions -> logits (B, V) of every sequence's last position, through
        the training-forward kernels; caches (nullable): every layer's q/k/v rows [0, T) are also left in its K/V cache."""
        NH, H = self._heads()

        def attend(l, h, wqkv):
            qkv = ops.gemm_nt(h, wqkv, self.act_dtype, split=self.split_bf16)
            if caches is not None:
                caches[l][:, :T].copy_(qkv.view(B, T, -1))
            return ops.attn_fwd(qkv, B, T, NH, H, H ** -0.5, 0.0, None, 0)[0]

        x = self._layers(x, ws, attend)
        return self._lm_logits(x.view(B, T, -1)[:, -1].contiguous(), w_lm, lm_bias)

    @torch.no_grad()
    def _prefill(self, idx, caches, ws, w_lm):
        """the prompt in ONE pass through the training-forward kernels (not one decode step per position): fills every layer's
        K/V cache rows [0, t0) and returns the logits (B, V) of the last prompt position -- the values the reference's full
        forward produces for it (the uncached path runs exactly these kernels)."""
        B, t0 = idx.shape
        x = ops.embed_fwd(idx, self.token_embedding_table.weight, self.position_embedding_table.weight).view(B * t0, -1)
        return self._forward_rows(x, B, t0, caches, ws, w_lm)

    def _kv_logits(self, prompt):
        """the host loop's second logits source: the prompt's prefill on the first call, then one K/V-cached step per token while
        the sequence fits the context window; once the window slides every position embedding shifts, the cache is void, and
        the source hands over to the full forward on the cropped window for good"""
        self._check_ids(prompt, None)
        kv = []                                   # (caches, ws, w_lm), made with the prefill

        def source(idx):
            t = idx.shape[1] - 1
            if t >= self.context_length:
                return self._window_logits(idx)
            if kv:
                return self._decode_step(idx[:, -1:].contiguous(), t, *kv)
            ws, w_lm = self._decode_weights()
            shape = (idx.shape[0], self.context_length, 3 * self.token_embedding_table.weight.shape[1])
            kv.extend(([torch.zeros(shape, dtype=self.act_dtype, device=idx.device) for _ in self.blocks], ws, w_lm))
            return self._prefill(idx.contiguous(), *kv)      # the whole prompt in one pass
        return source

    def generate(self, idx, max_new_tokens, generator: Optional[torch.Generator] = None, use_cache: bool = True, *,
                 sampler: str = "host", temperature: float = 1.0, top_k: Optional[int] = None, seed: Optional[int] = None,
                 top_p: Optional[float] = None, min_p: Optional[float] = None, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias=None, stop_tokens=None,
                 pad_token: Optional[int] = None, stop_poll: int = 64, prompt_lengths=None, return_lengths: bool = False,
                 return_logprobs: bool = False, top_logprobs: int = 0, best_of: int = 1):
        """ref: src/model.py:611-636.  While the sequence still fits the context window the per-layer K/V of the
        tokens seen so far are kept (training layout, [B, ctx, 3C]) and only the new position is computed; once the
        window starts to slide every position embedding shifts, the cache is void, and decoding continues exactly
        as the reference does (full forward on the cropped window).  Dropout is off in both paths only in eval()
        mode -- like the reference, train() mode samples with dropout through the uncached path.
        sampler / temperature / top_k / seed / top_p / min_p and the controls (repetition_penalty, presence_penalty,
        frequency_penalty, logit_bias, stop_tokens, pad_token, stop_poll; counts cover the whole sequence so far, prompt
        included and beyond the context window): as in _LM.generate.  sampler="device" in eval() mode with
        use_cache=True replays one captured graph per token (decode.DeviceDecoder): no host work inside the loop, and the same
        graphs for every setting of the sampler; a call with any control replays a second pair of graphs, captured once, whose
        sampler is dg_sample_rows_control.  prompt_lengths / return_lengths: as in _LM.generate; the graph-replayed path prefills
        idx[:, :min p_b] in one pass, the rows with longer prompts ride along through their remaining prompt tokens one step
        each, and a third pair of graphs, whose sampler is dg_sample_rows_ragged, is captured on the first such call.
        return_logprobs / top_logprobs / best_of: as in _LM.generate; the graph-replayed path replays scored twins of the mode's
        pair (the same steps with one dg_token_logprobs launch between the sampler and dg_state_advance), captured on the first
        scored call per mode; a call without them replays the graphs it always did.
        The document mask (set_doc_separator) is not applied: neither the decode kernels, the prefill nor the graphs know it, and
        the tokens are bit for bit those without a separator set; stop_tokens=[sep] ends a sample at the end of its document."""
        req = Sampling.checked(self.token_embedding_table.weight.shape[0], generator, sampler, temperature, top_k, seed, top_p, min_p,
                               repetition_penalty, presence_penalty, frequency_penalty, logit_bias, stop_tokens, pad_token, stop_poll,
                               prompt_lengths, tuple(getattr(idx, "shape", ())), return_lengths, return_logprobs, top_logprobs, best_of)
        T = idx.shape[1] if getattr(idx, "dim", lambda: 0)() == 2 else 0
        idx, done = req.enter(idx, max_new_tokens)
        if done is not None:
            return done
        cached = use_cache and not self.training
        if sampler == "device":
            out = (self._generate_device_cached if cached else self._generate_device)(idx, max_new_tokens, req)
        elif cached and req.span(idx.shape[1], 0)[0] < self.context_length:
            out = self._generate_host(idx, max_new_tokens, req, self._kv_logits(idx))
        else:
            out = self._generate_host(idx, max_new_tokens, req)
        return req.deliver(out, T) if req.scored else out

    # ------------------------------------------------------------------ graph-replayed decoding (sampler="device")
    def __getstate__(self):
        d = self.__dict__.copy()
        d.pop("_decoders", None)              # captured graphs and their buffers are rebuilt on demand, never copied or pickled
        return d

    @torch.no_grad()
    def _generate_device_cached(self, idx, max_new_tokens, req: Sampling, graph: bool = True):
        """eager one-pass prefill, sample, advance; then one step per token on the device position L: the K/V-cached step while
        L <= ctx, the full-window step after that.  graph=True replays the two captured graphs of decode.DeviceDecoder;
        graph=False launches the very same steps eagerly.  With a control the steps end in dg_sample_rows_control on the decoder's
        operands, and graph=True replays the decoder's second pair of graphs; with stop tokens the host reads lengths every
        req.poll tokens.  With prompt_lengths L starts at min p_b (the prefill is that of idx[:, :min p_b]; none if it does not fit
        the window), the steps end in dg_sample_rows_ragged, and graph=True replays the decoder's third pair."""
        from .decode import DeviceDecoder
        B, T = self._prompt_shape(idx)
        (t0, total), ctx = req.span(T, max_new_tokens), self.context_length
        key = (B, idx.device, self.act_dtype, self.split_bf16)
        decs = self.__dict__.setdefault("_decoders", {})
        dec = decs.get(key)
        if dec is None or dec.cap < total:
            dec = decs[key] = DeviceDecoder(self, B, idx.device, total)
        dec.refresh(self)                      # a generate() after an optimizer step sees the new weights
        mode = "ragged" if req.ragged else "plain" if req.ctl is None else "control"
        scored = req.scored
        if graph:
            dec.capture(mode, scored)
        state, params = self._decode_begin(idx, req, dec.ids, t0, graph=True)      # the decoder's block: four words, replayed or not
        dec.state.copy_(state)
        dec.params.copy_(params)
        if mode != "plain":
            dec.operands.begin(req.ctl, dec.ids, T, req.prompt_lengths, max_new_tokens)
        if scored:
            dec.begin_scores(req.top_logprobs)         # outside the graphs: zeros, sentinels and the top_n word
        lengths = dec.lengths if req.poll or req.ragged else None
        L = t0
        prefill = max_new_tokens > 0 and t0 < ctx
        if prefill:
            dec.tail(self._prefill(idx[:, :t0].contiguous(), dec.caches, dec.ws, dec.w_lm), mode, scored)
            L += 1
        while L < total and not (L > t0 and stop_poll_due(req.poll, L - t0, lengths)):
            dec.step(cached=prefill and L <= ctx, graph=graph, mode=mode, scored=scored)      # no prefill: the caches hold nothing to step on
            L += 1
        if scored:
            gen = make_generation(dec.ids, lengths, total, *dec.scores, req.top_logprobs)
            return Generation(*(t.clone() for t in gen))
        out = trim_to_longest(dec.ids, lengths, total, req.return_lengths)
        return (out[0].clone(), out[1]) if req.return_lengths else out.clone()


MODEL_CLASSES = OrderedDict(
    BigramLM=BigramLM,
    SingleHeadAttentionLM=SingleHeadAttentionLM,
    MultiHeadAttentionLM=MultiHeadAttentionLM,
    BlocksLM=BlocksLM,
    ResidualBlocksLM=ResidualBlocksLM,
    TransformerLM=TransformerLM,
)
