"""AdamW on the HIP kernel for the drop-in (autograd) path -- the reference's
``torch.optim.AdamW(model.parameters(), lr=..., betas=...)`` (src/train.py:121) with the same defaults
(eps 1e-8, weight_decay 1e-2, amsgrad off); parameters whose ``.grad`` is None are skipped entirely
(``ln_f``).  The graph-captured TrainEngine has its own flat-buffer optimizer step.

MI355X-first: on the first step the parameters that have a gradient are moved into ONE flat fp32 buffer (their
``.data`` become views of it, so ``state_dict()`` keeps working), with flat ``m`` / ``v`` / gradient buffers beside it:
a step is one fused copy of the gradients, one ``dg_adamw_step`` launch (which also moves the step counter on) instead of two
launches per parameter tensor (168 for the tiny TransformerLM).  With a process group the flat gradient is
all-reduced (SUM) first and the kernel applies 1 / world: data-parallel training for all six models.

max_grad_norm: global-norm clipping, ``torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)`` just before ``step()``,
over every parameter group, on the mean gradient over ranks.  ``step()`` then copies (and all-reduces) every group's gradient
first, computes one norm over all groups' flat gradients on the GPU and updates every group with the same coefficient, which the
AdamW launch applies: ``p.grad`` keeps the unclipped gradient (clip_grad_norm_ clips it in place).  ``last_grad_norm`` is the
pre-clip norm of the latest step, a device scalar.

ema_decay (with ema_warmup): an exponential moving average of the weights, one flat buffer per parameter group, moved on inside the
AdamW launch by the group's own step count (the recurrence of ``AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(d))``
updated after every ``step()``).  ``with optimizer.ema_weights():`` swaps the weights with their average for evaluation, sampling
or ``model.state_dict()``; ``state_dict()`` carries the averages under a top-level ``"ema"`` key (only when on).

skip_nonfinite / skip_grad_norm: the update guard (``torch.amp.GradScaler``'s found_inf skip, decided on the GPU with no host sync).
One norm is taken over all groups' flat gradients, with or without clipping; every group's AdamW launch reads the same guard word
and, when the norm is not finite (or above ``skip_grad_norm``), touches nothing: no group's parameters, moments, average or step
count move.  The sum of squares is taken in fp32, so a gradient element beyond 1.8e19 in magnitude reads as non-finite.
``last_step_applied`` is the latest decision (a device scalar), ``skipped_steps()`` the count; ``state_dict()`` carries a top-level
``"guard"`` key (only when on)."""
from __future__ import annotations

import contextlib
import math
from typing import Optional

import torch

from . import ops

_ALIGN = 64          # floats: every tensor starts on a 256-byte boundary of the flat buffer


def check_max_grad_norm(v) -> float:
    """a clipping threshold must be a finite number > 0 (None, for no clipping, is handled by the callers)"""
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"max_grad_norm must be a finite number > 0, got {v!r}") from None
    if not math.isfinite(f) or f <= 0.0:
        raise ValueError(f"max_grad_norm must be a finite number > 0, got {v!r}")
    return f


def check_accum_steps(v) -> int:
    """accum_steps (micro-batches per optimizer step) must be an integer >= 1: no bools, no floats (2.0 is a typo, not a count)"""
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"accum_steps must be an integer >= 1, got {v!r}")
    return int(v)


class _Flat:
    def __init__(self, params, device):
        self.key = tuple(id(p) for p in params)
        self.offsets, n = [], 0
        for p in params:
            self.offsets.append(n)
            n += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        self.n = n
        self.flat = torch.zeros(n, dtype=torch.float32, device=device)
        self.g = torch.zeros(n, dtype=torch.float32, device=device)
        self.m = torch.zeros(n, dtype=torch.float32, device=device)
        self.v = torch.zeros(n, dtype=torch.float32, device=device)
        self.t = ops.new_rng_state(0, device, 0)                 # word 2 = number of steps taken
        self.hyper = torch.zeros(5, dtype=torch.float32, device=device)
        self.hyper_host = None
        self.gviews = [self.g[o:o + p.numel()].view(p.shape) for o, p in zip(self.offsets, params)]
        self.ema = self.ema_hyper = None                         # AdamW(ema_decay=...): the moving average of flat, {decay, warmup}

    def view(self, buf, i, p):
        return buf[self.offsets[i]:self.offsets[i] + p.numel()].view(p.shape)


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, process_group=None, world_size: int = 1,
                 max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None, ema_warmup: bool = False,
                 skip_nonfinite: bool = False, skip_grad_norm: Optional[float] = None):
        self.max_grad_norm = None if max_grad_norm is None else check_max_grad_norm(max_grad_norm)
        self.ema_decay = ops.check_ema_options(ema_decay, ema_warmup)
        self.ema_warmup = bool(ema_warmup)
        self._ema_hyper = {}            # device -> {decay, warmup} there, made with the first flat group on that device
        self._in_ema = False
        self.guard_on, self._guard_limit_host = ops.check_guard_options(skip_nonfinite, skip_grad_norm)
        self.skip_grad_norm = None if skip_grad_norm is None else self._guard_limit_host
        self._guard = self._guard_limit = None      # device {apply, skipped, consecutive, spare} and the fp32 limit (after the first step)
        self._guard_loaded = None                   # counters of a loaded state_dict, written with the first step's allocation
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.process_group, self.world_size = process_group, int(world_size)
        self._flat = {}
        self._clip = None               # device {total_norm, coef, max_norm, 0} (clipping on, after the first step)
        self._clip_host = None
        self._norm_work = None

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """pre-clip global gradient norm of the latest step (0-d device tensor; None without clipping or before the first step)"""
        return None if self._clip is None else self._clip[0]

    @property
    def last_step_applied(self) -> Optional[torch.Tensor]:
        """1 if the latest step() applied its update, 0 if the guard skipped it (0-d device tensor; None without the guard or before
        the first step)"""
        return None if self._guard is None else self._guard[0]

    def skipped_steps(self) -> int:
        """steps the guard has skipped so far.  Synchronises."""
        if not self.guard_on:
            raise RuntimeError("skipped_steps: this optimizer was built without the update guard (AdamW(..., skip_nonfinite=True))")
        if self._guard is None:
            return 0 if self._guard_loaded is None else self._guard_loaded[0]
        return int(self._guard[1].item()) & 0xFFFFFFFF

    def consecutive_skips(self) -> int:
        """steps skipped in a row up to the latest one (0 after an applied update).  Synchronises."""
        if not self.guard_on:
            raise RuntimeError("consecutive_skips: this optimizer was built without the update guard (AdamW(..., skip_nonfinite=True))")
        if self._guard is None:
            return 0 if self._guard_loaded is None else self._guard_loaded[1]
        return int(self._guard[2].item()) & 0xFFFFFFFF

    def set_skip_grad_norm(self, limit: Optional[float]) -> None:
        """a new norm limit for the following steps, or None for non-finite gradients only"""
        if not self.guard_on:
            raise RuntimeError("set_skip_grad_norm: this optimizer was built without the update guard (AdamW(..., skip_nonfinite=True))")
        self._guard_limit_host = ops.check_guard_options(True, limit)[1]
        self.skip_grad_norm = None if limit is None else self._guard_limit_host
        if self._guard_limit is not None:
            self._guard_limit.fill_(self._guard_limit_host)

    def _adopt(self, gi: int, params) -> _Flat:
        old = self._flat.get(gi)
        dev = params[0].device
        fl = _Flat(params, dev)
        carry = {}
        if old is not None:                                      # the set of trained parameters changed: keep their moments
            carry = {pid: i for i, pid in enumerate(old.key)}
            fl.t.copy_(old.t)
        for i, p in enumerate(params):
            dst = fl.view(fl.flat, i, p)
            dst.copy_(p.data)
            p.data = dst
            if id(p) in carry:
                j = carry[id(p)]
                fl.view(fl.m, i, p).copy_(old.m[old.offsets[j]:old.offsets[j] + p.numel()].view(p.shape))
                fl.view(fl.v, i, p).copy_(old.v[old.offsets[j]:old.offsets[j] + p.numel()].view(p.shape))
        if self.ema_decay is not None:
            fl.ema = fl.flat.clone()                             # defined before the first step, which overwrites it (step word 0)
            if old is not None and old.ema is not None:          # the set of trained parameters changed: keep their averages
                for i, p in enumerate(params):
                    if id(p) in carry:
                        j = carry[id(p)]
                        fl.view(fl.ema, i, p).copy_(old.ema[old.offsets[j]:old.offsets[j] + p.numel()].view(p.shape))
            if dev not in self._ema_hyper:
                self._ema_hyper[dev] = ops.new_ema_hyper(self.ema_decay, self.ema_warmup, dev)
            fl.ema_hyper = self._ema_hyper[dev]
        self._flat[gi] = fl
        return fl

    def _ema_kw(self, fl: _Flat) -> dict:
        """what step() adds to its ops.adamw_step call: nothing without ema_decay (ops.adamw_step routes by what it is given)"""
        return {} if fl.ema is None else {"ema": fl.ema, "ema_hyper": fl.ema_hyper}

    def set_ema_decay(self, decay: float) -> None:
        if self.ema_decay is None:
            raise RuntimeError("set_ema_decay: this optimizer was built without a moving average (AdamW(..., ema_decay=...))")
        d = ops.check_ema_options(decay, self.ema_warmup)
        if d is None:
            raise ValueError("set_ema_decay: the decay must be a number in (0, 1)")
        self.ema_decay = d
        for t in self._ema_hyper.values():
            t[0:1].fill_(d)

    @contextlib.contextmanager
    def ema_weights(self):
        """`with optimizer.ema_weights():` -- the parameters hold their moving average inside (one dg_swap_f32 launch per flat
        group on entry, one on exit: the parameters are views of the flat buffers); step(), state_dict() and load_state_dict()
        raise RuntimeError inside.  Groups that have not taken a step yet have no average: their parameters stay as they are."""
        if self.ema_decay is None:
            raise RuntimeError("ema_weights: this optimizer was built without a moving average (AdamW(..., ema_decay=...))")
        self._refuse_in_ema("ema_weights()")
        flats = [fl for fl in self._flat.values() if fl.ema is not None]
        for fl in flats:
            ops.swap_(fl.flat, fl.ema)
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            for fl in flats:
                ops.swap_(fl.flat, fl.ema)

    def _refuse_in_ema(self, what: str) -> None:
        if self._in_ema:
            raise RuntimeError(f"{what} inside `with ema_weights()`: the weights are swapped with their moving average; leave the "
                               "context first")

    @torch.no_grad()
    def step(self, closure=None):
        self._refuse_in_ema("step()")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        scale = 1.0 / self.world_size if self.world_size > 1 else 1.0
        if self.max_grad_norm is None and not self.guard_on:
            for gi, group in enumerate(self.param_groups):
                fl = self._gather(gi, group)
                if fl is not None:
                    ops.adamw_step(fl.flat, fl.g, fl.m, fl.v, fl.hyper, fl.t, grad_scale=scale, advance=True, **self._ema_kw(fl))
            return loss
        # clipping / the guard: every group's (all-reduced) gradient first, then ONE norm over all of them, then every group's
        # update with its coefficient / its decision
        flats = [fl for fl in (self._gather(gi, group) for gi, group in enumerate(self.param_groups)) if fl is not None]
        if not flats:
            return loss
        dev = flats[0].g.device
        if self._clip is None or self._clip.device != dev:
            self._clip = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float32, device=dev)
            self._clip_host = None
        if self.max_grad_norm is not None and self._clip_host != self.max_grad_norm:
            self.max_grad_norm = check_max_grad_norm(self.max_grad_norm)
            self._clip[2:3].fill_(self.max_grad_norm)
            self._clip_host = self.max_grad_norm
        key = tuple(fl.n for fl in flats)
        if self._norm_work is None or self._norm_work[0] != key or self._norm_work[1].device != dev:
            self._norm_work = (key, ops.grad_norm_workspace([fl.g for fl in flats], dev))
        clip = {} if self.max_grad_norm is None else {"clip": self._clip[1:2]}
        guard_norm, guard_step = {}, {}
        if self.guard_on:
            if self._guard is None or self._guard.device != dev:
                old = self._guard
                self._guard = ops.new_update_guard(dev)
                self._guard_limit = torch.tensor([self._guard_limit_host], dtype=torch.float32, device=dev)
                if old is not None:
                    self._guard.copy_(old)
                elif self._guard_loaded is not None:
                    sk, cons = self._guard_loaded
                    self._guard.copy_(torch.tensor([0 if cons else 1, sk, cons, 0], dtype=torch.int32))
                self._guard_loaded = None
            guard_norm = {"guard": self._guard, "limit": self._guard_limit}
            guard_step = {"guard": self._guard}
        ops.grad_norm([fl.g for fl in flats], scale, None if self.max_grad_norm is None else self._clip[2:3], self._clip,
                      self._norm_work[1], **guard_norm)
        for fl in flats:
            ops.adamw_step(fl.flat, fl.g, fl.m, fl.v, fl.hyper, fl.t, grad_scale=scale, advance=True, **clip, **self._ema_kw(fl),
                           **guard_step)
        return loss

    def _gather(self, gi: int, group) -> Optional[_Flat]:
        """the group's flat buffers, current hyperparameters and gradient (all-reduced under data parallelism); None: no gradients"""
        params = [p for p in group["params"] if p.grad is not None]
        if not params:
            return None
        if any(not p.is_cuda for p in params):
            raise RuntimeError("drakegpt_amd.optim.AdamW updates GPU parameters only (no CPU path)")
        fl = self._flat.get(gi)
        if fl is None or fl.key != tuple(id(p) for p in params) or any(p.data.data_ptr() != fl.flat.data_ptr() + 4 * o
                                                                       for p, o in zip(params, fl.offsets)):
            fl = self._adopt(gi, params)
        hy = (group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"])
        if hy != fl.hyper_host:
            fl.hyper.copy_(torch.tensor(hy, dtype=torch.float32))
            fl.hyper_host = hy
        torch._foreach_copy_(fl.gviews, [p.grad for p in params])           # one fused launch
        if self.world_size > 1:
            import torch.distributed as dist
            dist.all_reduce(fl.g, op=dist.ReduceOp.SUM, group=self.process_group)
        return fl

    def is_finite(self) -> bool:
        """are the parameters and Adam's moments all finite?  (TrainEngine.is_finite for the autograd path: the sum-of-squares
        launch of the gradient norm over every group's flat buffers -- before a group's first step, over its parameters -- and
        one device round trip.)  Ask before a good checkpoint is replaced by a diverged run's."""
        ts = []
        for gi, group in enumerate(self.param_groups):
            fl = self._flat.get(gi)
            held = set(fl.key) if fl is not None else ()
            if fl is not None:
                ts += [fl.flat, fl.m, fl.v]
            ts += [p.detach().float().contiguous().clone() for p in group["params"] if id(p) not in held and p.numel()]
        if any(not t.is_cuda for t in ts):
            raise RuntimeError("drakegpt_amd.optim.AdamW updates GPU parameters only (no CPU path)")
        return ops.all_finite(ts)

    # ---- checkpointing: the moments and the step count live in the flat buffers, not in torch's per-parameter `state`; export /
    # import them in torch.optim.AdamW's own format (state[i] = {"step", "exp_avg", "exp_avg_sq"}) so that a resumed run keeps
    # its bias correction and moments, and a state_dict written by torch.optim.AdamW loads here (ref: src/train.py:121)
    def state_dict(self):
        self._refuse_in_ema("state_dict()")
        sd = super().state_dict()                   # param_groups with indices; `state` is empty (nothing lives there)
        state, base = {}, 0
        ema = {}
        for gi, group in enumerate(self.param_groups):
            fl = self._flat.get(gi)
            if fl is not None:
                idx = {id(p): base + j for j, p in enumerate(group["params"])}
                t = float(fl.t[2].item())
                by_id = {id(p): p for p in group["params"]}
                for i, pid in enumerate(fl.key):
                    p = by_id.get(pid)
                    if p is None:
                        continue
                    state[idx[pid]] = {"step": torch.tensor(t), "exp_avg": fl.view(fl.m, i, p).detach().clone(),
                                       "exp_avg_sq": fl.view(fl.v, i, p).detach().clone()}
                    if fl.ema is not None:
                        ema[idx[pid]] = fl.view(fl.ema, i, p).detach().clone()
            base += len(group["params"])
        sd["state"] = state
        if self.ema_decay is not None:              # only when on: without it the dict is torch.optim.AdamW's, key for key
            sd["ema"] = {"decay": self.ema_decay, "warmup": self.ema_warmup, "values": ema}
        if self.guard_on:                           # only when on, too
            sd["guard"] = {"skipped": self.skipped_steps(), "consecutive": self.consecutive_skips(), "limit": self.skip_grad_norm}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        self._refuse_in_ema("load_state_dict()")
        state = state_dict.get("state", {})
        ema = state_dict.get("ema")
        if (ema is not None) != (self.ema_decay is not None):
            raise ValueError(f"optimizer state: ema differs: saved {'present' if ema is not None else None!r}, this optimizer has "
                             f"ema_decay = {self.ema_decay!r}")
        if ema is not None:
            for k in ("decay", "warmup", "values"):
                if k not in ema:
                    raise ValueError(f"optimizer state: missing key ema.{k}")
            decay = ops.check_ema_options(ema["decay"], bool(ema["warmup"]))
            if decay is None or sorted(int(i) for i in ema["values"]) != sorted(int(i) for i in state):
                raise ValueError("optimizer state: ema.values must hold one average per parameter that has Adam moments")
            # what the loop below refuses, found before the file's decay is taken over: a refused load leaves the options as they were
            base = 0
            for group in self.param_groups:
                idx = [base + j for j in range(len(group["params"])) if (base + j) in state]
                if any(not group["params"][i - base].is_cuda for i in idx):
                    raise RuntimeError("drakegpt_amd.optim.AdamW updates GPU parameters only (no CPU path)")
                steps = sorted({int(float(state[i]["step"])) for i in idx})
                if len(steps) > 1:
                    raise ValueError("drakegpt_amd.optim.AdamW keeps ONE step count per parameter group; the state holds " + str(steps))
                base += len(group["params"])
        guard = state_dict.get("guard")
        if guard is not None and not self.guard_on:
            raise ValueError("optimizer state: guard differs: saved present, this optimizer has the update guard off")
        if guard is not None:
            for k in ("skipped", "consecutive", "limit"):
                if k not in guard:
                    raise ValueError(f"optimizer state: missing key guard.{k}")
            for k in ("skipped", "consecutive"):
                if isinstance(guard[k], bool) or not isinstance(guard[k], int) or not 0 <= guard[k] < (1 << 31):
                    raise ValueError(f"optimizer state: guard.{k} is {guard[k]!r}, expected an integer >= 0")
            ops.check_guard_options(True, guard["limit"])
        super().load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})
        if self.guard_on:      # (a file without the section: the guard was turned on mid-run, the counters start at 0)
            self._guard = self._guard_limit = None
            self._guard_loaded = (guard["skipped"], guard["consecutive"]) if guard is not None else None
            if guard is not None:
                self.set_skip_grad_norm(guard["limit"])
        if ema is not None:
            self.ema_decay, self.ema_warmup = decay, bool(ema["warmup"])
            for t in self._ema_hyper.values():
                t.copy_(torch.tensor([decay, 1.0 if self.ema_warmup else 0.0], dtype=torch.float32))
        base = 0
        for gi, group in enumerate(self.param_groups):
            have = [(j, p) for j, p in enumerate(group["params"]) if (base + j) in state]
            if have:
                params = [p for _, p in have]
                if any(not p.is_cuda for p in params):
                    raise RuntimeError("drakegpt_amd.optim.AdamW updates GPU parameters only (no CPU path)")
                self._flat.pop(gi, None)
                fl = self._adopt(gi, params)
                steps = set()
                for i, (j, p) in enumerate(have):
                    st = state[base + j]
                    fl.view(fl.m, i, p).copy_(st["exp_avg"].to(p.device, torch.float32))
                    fl.view(fl.v, i, p).copy_(st["exp_avg_sq"].to(p.device, torch.float32))
                    if ema is not None:
                        fl.view(fl.ema, i, p).copy_(ema["values"][base + j].to(p.device, torch.float32))
                    steps.add(int(float(st["step"])))
                if len(steps) != 1:
                    raise ValueError("drakegpt_amd.optim.AdamW keeps ONE step count per parameter group; the state holds " + str(sorted(steps)))
                fl.t.copy_(ops.new_rng_state(0, params[0].device, steps.pop()))
            base += len(group["params"])
