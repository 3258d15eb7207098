"""Training-state files: what TrainEngine.state_dict() / the harness write, and the optimizer-format mapping behind them.

Nothing here touches the GPU.  A training state is a nested dict of CPU tensors, ints, floats, strings, lists and None, so the
file loads with ``torch.load(..., weights_only=True)`` like every other file of this project:

    {"format": "drakegpt_amd.train_state", "version": 1,
     "model": {...}, "optimizer": {...}, "engine": {...}, "meta": {...}}          # TrainEngine.state_dict()

The harness (drakegpt_amd.train) wraps that in a dict of the same format / version with its own fields beside it.

The optimizer part is torch.optim.AdamW's own format.  The engine keeps Adam's moments in flat buffers whose layout is keyed by
region ("3.wqkv", "lm.w", "tok", ...: engine._build_layout); ``param_region`` says which rows of which region a reference
parameter name is, ``region_params`` is its inverse, and ``optimizer_state_from_regions`` / ``regions_from_optimizer_state``
move whole optimizer states between the two forms."""
from __future__ import annotations

import os
import re
import tempfile
from typing import Dict, List, Optional, Sequence, Tuple

import torch

Tensor = torch.Tensor
FORMAT = "drakegpt_amd.train_state"
VERSION = 1

_BLOCK_KEYS = (("sa_head.proj.weight", "wproj"), ("sa_head.proj.bias", "bproj"), ("ffwd.net.0.weight", "w1"), ("ffwd.net.0.bias", "b1"),
               ("ffwd.net.2.weight", "w2"), ("ffwd.net.2.bias", "b2"), ("ln1.weight", "ln1w"), ("ln1.bias", "ln1b"),
               ("ln2.weight", "ln2w"), ("ln2.bias", "ln2b"))
_TOP_KEYS = (("lm_head.weight", "lm.w"), ("lm_head.bias", "lm.b"), ("token_embedding_table.weight", "tok"),
             ("position_embedding_table.weight", "pos"), ("ln_f.weight", "lnf.w"), ("ln_f.bias", "lnf.b"))
_HEAD = re.compile(r"^blocks\.(\d+)\.sa_head\.heads\.(\d+)\.(query|key|value)\.weight$")
_BLOCK = re.compile(r"^blocks\.(\d+)\.(.+)$")
_QKV = {"query": 0, "key": 1, "value": 2}          # order of the three groups of NH heads inside a layer's packed [3 NH H, C] operand
UNTRAINED = ("lnf.w", "lnf.b")                     # regions the optimizer never touches (ln_f: no gradient)
# weight-decay groups: the kinds of parameter TrainEngine(no_decay=...) / train --no-decay keep out of weight decay, by region key
NO_DECAY_KINDS = {"bias": ("bproj", "b1", "b2", "lm.b"), "layernorm": ("ln1w", "ln1b", "ln2w", "ln2b", "lnf.w", "lnf.b"),
                  "embedding": ("tok", "pos")}


# ------------------------------------------------------------------------------------------ names <-> regions
def param_region(name: str, num_heads: int, head_size: int) -> Tuple[str, Optional[Tuple[int, int]]]:
    """(region key, rows) of a TransformerLM parameter under the reference's name.  rows is None when the parameter is the whole
    region, else the [lo, hi) rows of the layer's packed QKV matrix that hold this head's query / key / value weight."""
    m = _HEAD.match(name)
    if m:
        l, h, which = int(m.group(1)), int(m.group(2)), _QKV[m.group(3)]
        if h >= num_heads:
            raise KeyError(name)
        lo = (which * num_heads + h) * head_size
        return f"{l}.wqkv", (lo, lo + head_size)
    m = _BLOCK.match(name)
    if m:
        for ref, key in _BLOCK_KEYS:
            if m.group(2) == ref:
                return f"{int(m.group(1))}.{key}", None
        raise KeyError(name)
    for ref, key in _TOP_KEYS:
        if name == ref:
            return key, None
    raise KeyError(name)


def region_params(key: str, num_heads: int, head_size: int) -> List[Tuple[str, Optional[Tuple[int, int]]]]:
    """inverse of param_region: the reference parameter names inside a region, each with its rows (None: the whole region)"""
    for ref, k in _TOP_KEYS:
        if key == k:
            return [(ref, None)]
    l, _, k = key.partition(".")
    if not l.isdigit():
        raise KeyError(key)
    if k == "wqkv":
        out = []
        for which, i in _QKV.items():
            for h in range(num_heads):
                lo = (i * num_heads + h) * head_size
                out.append((f"blocks.{l}.sa_head.heads.{h}.{which}.weight", (lo, lo + head_size)))
        return out
    for ref, kk in _BLOCK_KEYS:
        if k == kk:
            return [(f"blocks.{l}.{ref}", None)]
    raise KeyError(key)


def check_no_decay(kinds) -> Tuple[str, ...]:
    """the sorted, de-duplicated kinds of a no_decay collection; ValueError for anything outside NO_DECAY_KINDS"""
    if isinstance(kinds, str):
        raise ValueError(f"no_decay must be a collection out of {sorted(NO_DECAY_KINDS)}, got the string {kinds!r}")
    try:
        kinds = list(kinds)
    except TypeError:
        raise ValueError(f"no_decay must be a collection out of {sorted(NO_DECAY_KINDS)}, got {kinds!r}") from None
    for k in kinds:
        if not isinstance(k, str) or k not in NO_DECAY_KINDS:
            raise ValueError(f"no_decay: {k!r} is not one of {sorted(NO_DECAY_KINDS)}")
    return tuple(sorted(set(kinds)))


def region_no_decay(key: str, kinds) -> bool:
    """is the region kept out of weight decay under these kinds?  ("3.b1" and "lm.b" are biases, "3.ln1w" a LayerNorm parameter)"""
    tail = key if key in ("lm.b", "lm.w", "lnf.w", "lnf.b") else key.rpartition(".")[2]
    return any(tail in NO_DECAY_KINDS[k] for k in kinds)


def split_param_names(names: Sequence[str], num_heads: int, head_size: int, kinds) -> Tuple[List[str], List[str]]:
    """(decayed, not decayed) parameter names, each in model order: the two parameter groups of a torch.optim.AdamW that does
    what TrainEngine(no_decay=kinds) does"""
    kinds = check_no_decay(kinds)
    groups: Tuple[List[str], List[str]] = ([], [])
    for name in names:
        groups[region_no_decay(param_region(name, num_heads, head_size)[0], kinds)].append(name)
    return groups


def rows(t: Tensor, span) -> Tensor:
    """the part of a region's tensor that param_region's second result names (None: all of it)"""
    return t if span is None else t[span[0]:span[1]]


def optimizer_state_from_regions(names: Sequence[str], regions: Dict[str, Tuple[Tensor, Tensor]], num_heads: int, head_size: int,
                                 step: int, lr: float, betas, eps: float, weight_decay: float, no_decay=()) -> dict:
    """what torch.optim.AdamW(model.parameters(), ...) would save: `names` are model.named_parameters()'s names in order,
    `regions` maps a region key to its (exp_avg, exp_avg_sq) tensors in the region's own shape.  A parameter whose region is
    absent from `regions` (ln_f) gets no state entry, as in torch.
    no_decay (kinds, see check_no_decay) not empty: what AdamW([{"params": decayed}, {"params": others, "weight_decay": 0.0}], ...)
    over split_param_names' two lists would save -- torch numbers the parameters group by group."""
    no_decay = check_no_decay(no_decay)
    split = split_param_names(names, num_heads, head_size, no_decay) if no_decay else (list(names), [])
    state = {}
    for i, name in enumerate(split[0] + split[1]):
        key, span = param_region(name, num_heads, head_size)
        if key not in regions:
            continue
        m, v = regions[key]
        state[i] = {"step": torch.tensor(float(step)), "exp_avg": rows(m, span).detach().cpu().clone(),
                    "exp_avg_sq": rows(v, span).detach().cpu().clone()}
    # the group as the installed torch writes it (its set of option keys changes between releases): ask torch itself
    dummy = [{"params": [torch.nn.Parameter(torch.zeros(1)) for _ in split[0]]}]
    if no_decay:
        dummy.append({"params": [torch.nn.Parameter(torch.zeros(1)) for _ in split[1]], "weight_decay": 0.0})
    groups = torch.optim.AdamW(dummy, lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                               weight_decay=float(weight_decay)).state_dict()["param_groups"]
    return {"state": state, "param_groups": groups}


def regions_from_optimizer_state(sd: dict, names: Sequence[str], num_heads: int, head_size: int, no_decay=()):
    """inverse of optimizer_state_from_regions, for a dict written by it, by torch.optim.AdamW or by drakegpt_amd.optim.AdamW
    over the same model: ({region key: (exp_avg, exp_avg_sq)}, step, {"lr", "betas", "eps", "weight_decay"}).  Raises ValueError
    if the parameters disagree about the step count, if the state does not fit `names`, or if a packed QKV region is only partly
    present.  no_decay not empty: the dict must hold the two groups of split_param_names (the second with weight_decay 0 and
    otherwise the first one's options); "weight_decay" is then the first group's."""
    no_decay = check_no_decay(no_decay)
    groups = sd["param_groups"]
    if len(groups) != (2 if no_decay else 1):
        raise ValueError(f"optimizer state: expected {'two parameter groups' if no_decay else 'one parameter group'}, found {len(groups)}")
    g = groups[0]
    if no_decay:
        split = split_param_names(names, num_heads, head_size, no_decay)
        g1 = groups[1]
        if list(g["params"]) != list(range(len(split[0]))) or list(g1["params"]) != list(range(len(split[0]), len(names))):
            raise ValueError(f"optimizer state: the groups list {len(g['params'])} + {len(g1['params'])} parameters, no_decay = "
                             f"{list(no_decay)} splits the model's {len(names)} into {len(split[0])} + {len(split[1])}")
        if float(g1["weight_decay"]) != 0.0:
            raise ValueError(f"optimizer state: the second group has weight_decay {g1['weight_decay']!r}, expected 0")
        for opt in ("lr", "betas", "eps"):
            if (tuple(g[opt]) if opt == "betas" else g[opt]) != (tuple(g1[opt]) if opt == "betas" else g1[opt]):
                raise ValueError(f"optimizer state: the two groups differ in {opt}: {g[opt]!r} and {g1[opt]!r}")
        names = split[0] + split[1]
    elif list(g["params"]) != list(range(len(names))):
        raise ValueError(f"optimizer state: the group lists {len(g['params'])} parameters, the model has {len(names)}")
    state = sd["state"]
    steps = sorted({int(float(st["step"])) for st in state.values()})
    if len(steps) > 1:
        raise ValueError(f"optimizer state: the parameters disagree about the step count: {steps}")
    parts: Dict[str, list] = {}
    for i, st in state.items():
        i = int(i)
        if not 0 <= i < len(names):
            raise ValueError(f"optimizer state: entry {i} is outside the model's {len(names)} parameters")
        key, rows = param_region(names[i], num_heads, head_size)
        parts.setdefault(key, []).append((rows, st["exp_avg"].detach().cpu().float(), st["exp_avg_sq"].detach().cpu().float()))
    regions = {}
    for key, lst in parts.items():
        if lst[0][0] is None:
            regions[key] = (lst[0][1].clone(), lst[0][2].clone())
            continue
        lst.sort(key=lambda e: e[0][0])
        if [e[0] for e in lst] != [(k * head_size, (k + 1) * head_size) for k in range(3 * num_heads)]:
            raise ValueError(f"optimizer state: region {key} needs the query / key / value state of all {num_heads} heads")
        regions[key] = (torch.cat([e[1] for e in lst]), torch.cat([e[2] for e in lst]))
    hyper = {"lr": float(g["lr"]), "betas": (float(g["betas"][0]), float(g["betas"][1])), "eps": float(g["eps"]),
             "weight_decay": float(g["weight_decay"])}
    return regions, (steps[0] if steps else 0), hyper


# ------------------------------------------------------------------------------------------ files
def check_format(obj, what: str = "training state") -> None:
    if not isinstance(obj, dict):
        raise ValueError(f"{what}: expected a dict, found {type(obj).__name__}")
    for field, own in (("format", FORMAT), ("version", VERSION)):
        if field not in obj:
            raise ValueError(f"{what}: missing key {field!r}")
        if obj[field] != own:
            raise ValueError(f"{what}: {field} is {obj[field]!r}, this package reads {own!r}")


def check_compat(saved_meta: dict, own_meta: dict, what: str = "meta") -> None:
    """every field of own_meta must be present in saved_meta with the same value; ValueError names the field and both values"""
    for field, own in own_meta.items():
        if field not in saved_meta:
            raise ValueError(f"training state: missing key {what}.{field}")
        saved = saved_meta[field]
        if isinstance(own, (tuple, list)):
            same = isinstance(saved, (tuple, list)) and list(saved) == list(own)
        else:
            same = type(saved) is type(own) and saved == own
        if not same:
            raise ValueError(f"training state: {what}.{field} differs: saved {saved!r}, this run has {own!r}")


def check_ema_meta(saved_meta: dict, own: bool) -> None:
    """whether a moving average of the weights is kept must agree in both directions: meta["ema"] is written (True) only by an
    engine that keeps one, so a file from before it existed reads as off"""
    saved = saved_meta.get("ema", False)
    if not isinstance(saved, bool) or saved != bool(own):
        raise ValueError(f"training state: meta.ema differs: saved {saved!r}, this run has {bool(own)!r}")


def check_ema_state(section, own: bool, n: int):
    """the "ema" section of an engine / optimizer state ({"decay", "warmup", "values"}) against a run that keeps an average (own)
    of n floats or does not; returns None or (decay, warmup, values).  ValueError names the field."""
    from .ops import check_ema_options
    if (section is not None) != bool(own):
        raise ValueError(f"training state: engine.ema differs: saved {'present' if section is not None else None!r}, this run has "
                         f"{'a moving average' if own else None!r}")
    if section is None:
        return None
    if not isinstance(section, dict):
        raise ValueError(f"training state: engine.ema is a {type(section).__name__}, expected a dict")
    for k in ("decay", "warmup", "values"):
        if k not in section:
            raise ValueError(f"training state: missing key engine.ema.{k}")
    if not isinstance(section["warmup"], bool):
        raise ValueError(f"training state: engine.ema.warmup is {section['warmup']!r}, expected a bool")
    try:
        decay = check_ema_options(section["decay"], section["warmup"])
    except ValueError as err:
        raise ValueError(f"training state: engine.ema.decay: {err}") from None
    if decay is None:
        raise ValueError("training state: engine.ema.decay is None")
    values = section["values"]
    if not isinstance(values, Tensor) or values.dtype != torch.float32 or tuple(values.shape) != (n,):
        raise ValueError(f"training state: engine.ema.values is {getattr(values, 'dtype', type(values).__name__)} "
                         f"{tuple(getattr(values, 'shape', ()))}, expected float32 {(n,)}")
    return decay, section["warmup"], values


def check_guard_meta(saved_meta: dict, own: bool) -> None:
    """meta["update_guard"] is written (True) only by an engine with the update guard on.  A guarded file is refused by an engine
    without the guard (its data word and its optimizer word may differ, and that engine has one word); an unguarded file loads
    into a guarded engine (the guard can be turned on mid-run), as does a guarded file."""
    saved = saved_meta.get("update_guard", False)
    if not isinstance(saved, bool):
        raise ValueError(f"training state: meta.update_guard is {saved!r}, expected a bool")
    if saved and not own:
        raise ValueError(f"training state: meta.update_guard differs: saved {saved!r}, this run has {bool(own)!r} (the file keeps "
                         "a data word and an optimizer word that may differ; load it into an engine with the update guard on)")


def check_guard_state(section, saved_meta: dict, own: bool, step_word: int):
    """the "guard" section of an engine state ({"skipped", "consecutive", "limit", "opt_step"}) against a run with the update
    guard on (own) or off; returns None (own off) or (opt_step, skipped, consecutive, limit, restore_limit).  An unguarded file
    into a guarded run: opt_step = step_word (None is returned for it: the caller knows its own word), counters 0, the run keeps
    its limit.  ValueError names the field."""
    from .ops import check_guard_options
    check_guard_meta(saved_meta, own)
    saved = bool(saved_meta.get("update_guard", False))
    if saved != (section is not None):
        raise ValueError(f"training state: engine.guard is {'present' if section is not None else None!r}, meta.update_guard says {saved!r}")
    if not own:
        return None
    if section is None:
        return None, 0, 0, None, False
    if not isinstance(section, dict):
        raise ValueError(f"training state: engine.guard is a {type(section).__name__}, expected a dict")
    for k in ("skipped", "consecutive", "limit", "opt_step"):
        if k not in section:
            raise ValueError(f"training state: missing key engine.guard.{k}")
    vals = []
    for k in ("opt_step", "skipped", "consecutive"):
        x = section[k]
        if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x < (1 << 32):
            raise ValueError(f"training state: engine.guard.{k} is {x!r}, expected an integer in [0, 2^32)")
        vals.append(x)
    if vals[2] > vals[1]:
        raise ValueError(f"training state: engine.guard.consecutive is {vals[2]}, more than engine.guard.skipped = {vals[1]}")
    if vals[0] > step_word:
        raise ValueError(f"training state: engine.guard.opt_step is {vals[0]}, more than engine.step_word = {step_word}")
    try:
        check_guard_options(True, section["limit"])
    except ValueError as err:
        raise ValueError(f"training state: engine.guard.limit: {err}") from None
    return vals[0], vals[1], vals[2], section["limit"], True


def save_train_state(path: str, obj: dict) -> None:
    """write to a temporary file in the same directory, then os.replace: the previous file stays intact until the new one is
    complete, and a failure leaves no temporary file behind"""
    check_format(obj)
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(dir=d, prefix=os.path.basename(path) + ".", suffix=".tmp")
    os.close(fd)
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def load_train_state(path: str) -> dict:
    obj = torch.load(path, map_location="cpu", weights_only=True)
    check_format(obj, f"training state {path}")
    return obj
