"""Training harness -- the reference's src/train.py on the HIP path.

    python -m drakegpt_amd.train --model TransformerLM --scale --data path/to/text.txt [--iters N]
    python -m torch.distributed.run --nproc-per-node 8 -m drakegpt_amd.train --model TransformerLM --scale ...

Data parallel semantics (weak scaling, as BASELINE.json configs[3] "global batch = 8 x local"): every rank trains the preset's
batch_size rows, the global batch is batch_size * world_size drawn by ONE seeded CPU generator (every rank draws all of it and
keeps its rows), the gradient is the mean over the global batch, and the learning rate is NOT rescaled -- the reference has a
single fixed batch of batch_size rows, so a world_size > 1 run is a different (larger-batch) optimisation problem by design.

Kept from the reference (src/train.py): build_model's per-model constructor arguments (:31-57),
evaluate_loss (eval mode, mean of eval_iters batch losses on train and val, :61-75), get_model_path
naming (:77-83), AdamW(lr=base_lr, betas) (:121), CyclicLR(base_lr, max_lr, step_size_up=5,
triangular) stepped once per evaluation (:122-126,162), seed 42 (:86), the step order
forward -> zero_grad -> backward -> step (:146-151), the final 100-token sample (:174-178) and the
state_dict checkpoint (:181-183).  Differences, on purpose: the selected preset
is used everywhere (batch shape and learning rates too), flags are real booleans, wandb is replaced
by JSON lines on stdout, and without --data a synthetic uniform char corpus stands in for the
Kaggle download.

Added beside the reference's loop, all off by default: --grad-clip, --accum-steps, --save-every / --resume, and --lr-schedule /
--warmup-steps / --min-lr / --no-decay: a rate per optimizer step over --iters steps (looked up on the GPU from a table on the
engine path, set as group["lr"] on the autograd path) and parameters kept out of weight decay.  The default `reference`
schedule is the CyclicLR stepped at evaluations described above.  --label-smoothing / --z-loss set the training objective
(inside the loss-head kernels, both paths); evaluation lines keep the plain cross entropy.  --ema-decay [--ema-warmup] keeps an
exponential moving average of the weights inside the AdamW launch (both paths): every evaluation line gains val_loss_ema (the
averaged weights on val_loss's own batches), the final sample is drawn from the average and it is saved as <name>.ema.pt beside
the raw checkpoint.  --skip-nonfinite / --skip-grad-norm X turn the update guard on (both paths): a step whose global gradient
norm is not finite (or above X), or -- engine path -- whose loss is not finite, skips its optimizer update on the GPU and the run
goes on with the next batch; evaluation lines gain "skipped", and a run that has skipped more than --max-consecutive-skips updates
in a row ends with a RuntimeError (checked where the harness synchronises anyway: at evaluation lines and before a save).  The
staged per-step LR table follows applied updates (a skipped step does not use up an entry); the `reference` schedule and the
autograd path's per-iteration rates keep counting iterations.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import os
import time
from typing import Optional

import torch

from . import checkpoint as CK
from . import dist as ddist
from . import schedules
from .config import DRAKE_VOCAB_SIZE, PARAMS, PRESETS, SCALE_PARAMS, TRAIN
from .model import MODEL_CLASSES, model_params
from .ops import check_ema_options, check_guard_options, check_loss_options
from .optim import check_accum_steps
from .preprocessing import draw_offsets, encode_text, get_mapper, load_train_val_data, split_train_val


def build_model(model_name: str, scale: bool, params: dict, scale_params: dict, vocab_size: int, device, precision: str = "fp32"):
    """ref: src/train.py:16-59 -- returns (model, model_config, params)."""
    if scale:
        params = scale_params
    if model_name not in MODEL_CLASSES:
        raise KeyError(f"unknown model {model_name!r}; choose from {list(MODEL_CLASSES)}")
    C, T = params["embedding_dim"], params["context_length"]
    cfg = {
        "BigramLM": dict(vocab_size=vocab_size),
        "SingleHeadAttentionLM": dict(vocab_size=vocab_size, embedding_dim=C, context_length=T, head_size=params["head_size"]),
        "MultiHeadAttentionLM": dict(vocab_size=vocab_size, embedding_dim=C, context_length=T, head_size=params["head_size"],
                                     num_heads=params["num_heads"]),
        "BlocksLM": dict(vocab_size=vocab_size, embedding_dim=C, context_length=T, num_heads=params["num_heads"],
                         num_layers=params["num_layers"]),
        "ResidualBlocksLM": dict(vocab_size=vocab_size, embedding_dim=C, context_length=T, num_heads=params["num_heads"],
                                 num_layers=params["num_layers"]),
        "TransformerLM": dict(vocab_size=vocab_size, embedding_dim=C, context_length=T, num_heads=params["num_heads"],
                              num_layers=params["num_layers"], dropout=params["dropout"]),
    }[model_name]
    model = MODEL_CLASSES[model_name](**cfg, precision=precision).to(device)
    return model, cfg, params


def no_decay_groups(model, kinds):
    """two torch-style parameter groups for the autograd path: everything else, then (weight_decay 0) the parameters `kinds`
    keeps out of weight decay -- by module type: Linear biases, LayerNorm weights and biases, Embedding tables"""
    kinds = CK.check_no_decay(kinds)
    types = {"bias": torch.nn.Linear, "layernorm": torch.nn.LayerNorm, "embedding": torch.nn.Embedding}
    skip = set()
    for mod in model.modules():
        for kind in kinds:
            if isinstance(mod, types[kind]):
                ps = [mod.bias] if kind == "bias" else list(mod.parameters(recurse=False))
                skip.update(id(p) for p in ps if p is not None)
    ps = list(model.parameters())
    return [{"params": [p for p in ps if id(p) not in skip]}, {"params": [p for p in ps if id(p) in skip], "weight_decay": 0.0}]


def get_model_path(dir, model_name: str, scale: bool) -> str:
    """ref: src/train.py:77-83"""
    return os.path.join(dir, f"{model_name}_scaled.pt" if scale else f"{model_name}.pt")


def cyclic_lr(step_count: int, base_lr: float, max_lr: float, step_size_up: int = 5) -> float:
    """torch CyclicLR(mode='triangular', cycle_momentum=False) after `step_count` scheduler steps"""
    total = 2.0 * step_size_up
    cycle = math.floor(1 + step_count / total)
    x = 1.0 + step_count / total - cycle
    ratio = step_size_up / total
    scale = x / ratio if x <= ratio else (x - 1) / (ratio - 1)
    return base_lr + (max_lr - base_lr) * scale


@torch.no_grad()
def evaluate_loss(train_data, val_data, model, eval_iters, context_length, batch_size, device, engine=None, generator=None,
                  drawn=None, offsets=None):
    """ref: src/train.py:61-75.  `model` must be in eval mode; batches are drawn as get_batch does.
    drawn: a dict that receives the window offsets of every split, [eval_iters, batch_size].  offsets: such a dict -- the splits
    it names are evaluated, on those offsets, and nothing is drawn (--ema-decay: the averaged weights on val_loss's batches)."""
    from . import ops
    out = {}
    for name, data in (("train", train_data), ("val", val_data)):
        if offsets is not None and name not in offsets:
            continue
        given = None if offsets is None else offsets[name]
        if engine is not None and data.is_cuda:
            # same draws in the same order as the loop below, staged once; the engine replays a captured forward per batch
            offs = given if given is not None else torch.stack([draw_offsets(len(data), context_length, batch_size, generator)
                                                                for _ in range(eval_iters)])
            if drawn is not None:
                drawn[name] = offs
            out[name] = engine.eval_losses(data, offs.to(device)).mean().cpu()
            continue
        losses = torch.zeros(eval_iters)
        rows = []
        for it in range(eval_iters):
            rows.append(given[it] if given is not None else draw_offsets(len(data), context_length, batch_size, generator))
            ix = rows[-1].to(device)
            x, y = ops.batch_gather(data, ix, context_length)
            loss = engine.eval_loss(x, y) if engine is not None else model(x, y)[1]
            losses[it] = loss.item()
        if drawn is not None:
            drawn[name] = torch.stack(rows)
        out[name] = losses.mean()
    return out


def engine_loop(engine, n_train: int, T: int, B: int, rank: int, world: int, iters: int, eval_interval: int, on_eval, device,
                generator: Optional[torch.Generator] = None, accum_steps: int = 1, start: int = 0) -> None:
    """The training iterations of ref: src/train.py:141-172 on the engine path.  The reference draws one randint(len(data) - T,
    (B,)) per step from the global CPU generator and, every eval_interval steps, 2 * eval_iters more inside evaluate_loss --
    the SAME generator.  Here the offsets of all steps up to the next evaluation are drawn in one go (same draws, same order:
    a stage never crosses an evaluation) and staged in HBM once (TrainEngine.stage_offsets): the captured step finds its own row
    through the device-side step counter, so a step is one graph launch and nothing else.
    `on_eval(it)` runs after step `it` when (it + 1) % eval_interval == 0.
    accum_steps = K > 1 (an engine built with the same accum_steps): an iteration is one optimizer step on K micro-batches; it
    draws K blocks of B * world offsets, in the order a loop of K get_batch calls would, so a stage holds K * n rows and
    `iters` / `eval_interval` count optimizer steps.
    start > 0: a resumed run -- iterations start .. iters - 1.  Its first stage runs to the next evaluation boundary, which are
    the rows (and draws) an uninterrupted run would still have had staged there."""
    for it in range(start, iters):
        if it % eval_interval == 0 or it == start:
            n = min(eval_interval - it % eval_interval, iters - it)
            engine.stage_offsets(torch.stack([ddist.shard_rows(draw_offsets(n_train, T, B * world, generator), rank, world)
                                              for _ in range(n * accum_steps)]))
        engine.step()
        if (it + 1) % eval_interval == 0:
            on_eval(it)
    engine.check_status()         # end of the run: a timed-out dW hand-over must not end in a saved checkpoint


LR_SCHEDULES = ("reference", "constant", "warmup-cosine", "warmup-linear", "cyclic")


def _no_decay_arg(text: str):
    """--no-decay bias,layernorm -> ("bias", "layernorm")"""
    try:
        return CK.check_no_decay([k.strip() for k in text.split(",") if k.strip()])
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def lr_values(args, base_lr: float, max_lr: float):
    """the rate of every optimizer step 0 .. --iters - 1 under --lr-schedule (None for `reference`, which is stepped at evaluations)"""
    if args.lr_schedule == "reference":
        return None
    if args.lr_schedule == "constant":
        return schedules.constant(base_lr, max(int(args.iters), 1))
    if args.lr_schedule == "cyclic":
        return schedules.cyclic(base_lr, max_lr, 5, max(int(args.iters), 1))
    form = schedules.warmup_cosine if args.lr_schedule == "warmup-cosine" else schedules.warmup_linear
    return form(max_lr, args.warmup_steps, args.iters, args.min_lr)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Train a DrakeGPT language model on MI355X")
    ap.add_argument("--model", default="TransformerLM", choices=list(MODEL_CLASSES))
    ap.add_argument("--scale", action="store_true", help="use SCALE_PARAMS (ref: --scale True)")
    ap.add_argument("--preset", default=None, choices=list(PRESETS), help="overrides --scale.  Under torch.distributed.run the "
                    "preset's batch_size is PER RANK (global batch = batch_size * world_size, learning rate unchanged)")
    ap.add_argument("--no-save", action="store_true")
    ap.add_argument("--data", default=None, help="UTF-8 text file (the reference's data/input.txt): tokenised and split 90/10 on "
                    "the fly, or -- with --train-data/--val-data -- only the source of the char mapper (ref: src/train.py:94-100)")
    ap.add_argument("--train-data", default=None, help="train_data.pt written by drakegpt_amd.preprocessing.get_train_val_data "
                    "(or the reference's src/preprocessing.py): 1-D int64 token tensor")
    ap.add_argument("--val-data", default=None, help="val_data.pt, same format")
    ap.add_argument("--iters", type=int, default=TRAIN["iters"])
    ap.add_argument("--eval-interval", type=int, default=TRAIN["eval_interval"])
    ap.add_argument("--eval-iters", type=int, default=TRAIN["eval_iters"])
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32", "fp8", "bf16x3"])
    ap.add_argument("--model-dir", default="model")
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--sampler", default="host", choices=["host", "device"], help="who draws the tokens of the sample printed at the "
                    "end: torch.multinomial on the host CPU generator (the reference's stream), or the GPU sampler kernel (no host "
                    "work per token)")
    ap.add_argument("--temperature", type=float, default=1.0, help="sampling temperature of that sample (0 = greedy)")
    ap.add_argument("--top-k", type=int, default=None, help="keep only the k most likely tokens of that sample (default: off)")
    ap.add_argument("--top-p", type=float, default=None, help="nucleus filter of that sample: keep the most likely tokens whose mass "
                    "reaches this share, in (0, 1] (default: off)")
    ap.add_argument("--min-p", type=float, default=None, help="keep only tokens at least this many times as likely as the best one, "
                    "in [0, 1] (default: off)")
    ap.add_argument("--repetition-penalty", type=float, default=1.0, metavar="R", help="of that sample: divide (multiply, when "
                    "negative) the logit of every token already in the sequence by R (default 1: off)")
    ap.add_argument("--presence-penalty", type=float, default=0.0, metavar="A", help="subtract A from the logit of every token "
                    "already in the sequence (default 0: off)")
    ap.add_argument("--frequency-penalty", type=float, default=0.0, metavar="F", help="subtract F per earlier occurrence of a token "
                    "from its logit (default 0: off)")
    ap.add_argument("--stop-token", type=int, action="append", default=None, metavar="ID", help="end the sample at this token id "
                    "(repeatable, up to 8; default: none)")
    ap.add_argument("--sample-logprobs", action="store_true", help="after the sample, print the mean log-probability the model gave "
                    "its tokens and their perplexity (generate(return_logprobs=True): the raw distribution, whatever the filters)")
    ap.add_argument("--top-logprobs", type=int, default=0, metavar="N", help="with the sample's log-probabilities, also collect the N "
                    "most likely tokens per position (0..20) and print how often the sampled token was the most likely one")
    ap.add_argument("--best-of", type=int, default=1, metavar="N", help="draw N samples and keep the one with the highest mean "
                    "log-probability (pads with --stop-token's first id, else 0)")
    ap.add_argument("--grad-clip", type=float, default=None, metavar="MAX_NORM",
                    help="clip the gradient to this global 2-norm before every AdamW step (ref: clip_grad_norm_; default: off); each "
                    "evaluation line then also reports the last step's pre-clip norm as grad_norm")
    ap.add_argument("--accum-steps", type=int, default=1, metavar="K",
                    help="gradient accumulation: K micro-batches of batch_size rows per AdamW step (the effective batch is K * "
                    "batch_size * world_size; --iters and --eval-interval count optimizer steps; default 1)")
    ap.add_argument("--lr-schedule", default="reference", choices=list(LR_SCHEDULES),
                    help="reference (default): the reference's CyclicLR(base_lr, max_lr, step_size_up=5), stepped once per evaluation.  "
                    "The others give every optimizer step its own rate over --iters steps, looked up on the GPU from a table staged "
                    "once: constant (the preset's base_lr), warmup-cosine / warmup-linear (--warmup-steps of linear warm-up to the "
                    "preset's max_lr, then a cosine / a straight line down to --min-lr at the last step), cyclic (that CyclicLR "
                    "stepped after every optimizer step)")
    ap.add_argument("--warmup-steps", type=int, default=0, metavar="N", help="warm-up steps of warmup-cosine / warmup-linear: step s "
                    "< N trains at max_lr * (s + 1) / N (default 0; --iters must exceed N + 1)")
    ap.add_argument("--min-lr", type=float, default=0.0, metavar="X", help="the rate warmup-cosine / warmup-linear end on (default 0)")
    ap.add_argument("--no-decay", type=_no_decay_arg, default=(), metavar="KINDS",
                    help="comma-separated kinds of parameter kept out of weight decay: bias (every Linear bias), layernorm (LayerNorm "
                    "weights and biases), embedding (the token and position tables); default: none, every parameter decays")
    ap.add_argument("--label-smoothing", type=float, default=0.0, metavar="E",
                    help="label smoothing of the training objective, in [0, 1) (F.cross_entropy's label_smoothing; default 0: off).  "
                    "Evaluation lines keep reporting the plain cross entropy")
    ap.add_argument("--z-loss", type=float, default=0.0, metavar="Z",
                    help="add Z * logsumexp(logits)^2 per row to the training objective (default 0: off; not with the fp8 loss head: "
                    "--precision fp8 at a large vocabulary)")
    ap.add_argument("--ignore-token", type=int, default=None, metavar="ID",
                    help="leave every position whose target is token ID out of the loss, in training and in the evaluation lines; each "
                    "batch's mean is over the targets that remain (F.cross_entropy's ignore_index; default: off).  A resumed run must "
                    "repeat it; not with the fp8 loss head (--precision fp8 at a large vocabulary)")
    ap.add_argument("--doc-separator", default=None, metavar="TOKEN",
                    help="document-masked attention: a document of the packed corpus ends with TOKEN and no token attends across it, in "
                    "training and in the evaluation lines (default: off).  TOKEN is an integer token id, or a single character looked "
                    "up in the tokenizer's table (needs --data).  Sampling does not apply the mask.  Often combined with --ignore-token")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the weights, ema += (w - ema) * (1 - D) after every optimizer step, "
                    "in (0, 1) (default: off).  Evaluation lines gain val_loss_ema, the final sample is drawn from the average and "
                    "it is saved as <name>.ema.pt beside the checkpoint")
    ap.add_argument("--ema-warmup", action="store_true", help="with --ema-decay: step s averages with min(D, (s + 1) / (s + 10))")
    ap.add_argument("--skip-nonfinite", action="store_true",
                    help="the update guard: skip the optimizer update of a step whose gradient norm (engine path: or loss) is not "
                    "finite, on the GPU, and go on with the next batch (default: off).  Evaluation lines gain skipped")
    ap.add_argument("--skip-grad-norm", type=float, default=None, metavar="X",
                    help="the update guard with a limit: also skip a step whose global gradient norm exceeds X (implies "
                    "--skip-nonfinite; default: off)")
    ap.add_argument("--max-consecutive-skips", type=int, default=25, metavar="N",
                    help="with the update guard: end the run (RuntimeError) once more than N updates in a row were skipped, checked at "
                    "evaluation lines and before a save (default 25)")
    ap.add_argument("--save-every", type=int, default=None, metavar="N",
                    help="write the full training state (weights, optimizer, counters, generator: everything --resume needs) after "
                    "the evaluation of every N-th iteration and after the last one; N must be a multiple of --eval-interval "
                    "(default: off)")
    ap.add_argument("--state-path", default=None, help="where --save-every writes (default: <model-dir>/<model>[_scaled].state.pt)")
    ap.add_argument("--resume", default=None, metavar="PATH", help="continue the run whose training state is in PATH; --iters stays "
                    "the total number of iterations")
    return ap


def parse_args(argv=None):
    """build_parser().parse_args plus the checks that span several flags"""
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.lr_schedule not in ("warmup-cosine", "warmup-linear") and (args.warmup_steps != 0 or args.min_lr != 0.0):
        ap.error(f"--warmup-steps and --min-lr go with --lr-schedule warmup-cosine or warmup-linear, not {args.lr_schedule}")
    if args.lr_schedule != "reference":
        try:
            lr_values(args, 1.0, 1.0)          # (the rates come from the preset later: the shape is checked here)
        except ValueError as e:
            ap.error(f"--lr-schedule {args.lr_schedule}: {e} (total is --iters, warmup is --warmup-steps)")
    try:
        args.label_smoothing, args.z_loss = check_loss_options(args.label_smoothing, args.z_loss)
    except ValueError as e:
        ap.error(f"--label-smoothing / --z-loss: {e}")
    try:
        args.ignore_token = check_loss_options(ignore_index=args.ignore_token)[2]
    except ValueError as e:
        ap.error(f"--ignore-token: {e}")
    try:
        args.ema_decay = check_ema_options(args.ema_decay, args.ema_warmup)
    except ValueError as e:
        ap.error(f"--ema-decay / --ema-warmup: {e}")
    try:
        args.skip_nonfinite = check_guard_options(bool(args.skip_nonfinite), args.skip_grad_norm)[0]
    except ValueError as e:
        ap.error(f"--skip-nonfinite / --skip-grad-norm: {e}")
    if args.max_consecutive_skips < 0:
        ap.error(f"--max-consecutive-skips {args.max_consecutive_skips} must be >= 0")
    if args.save_every is not None and (args.save_every < 1 or args.save_every % args.eval_interval):
        ap.error(f"--save-every {args.save_every} must be a positive multiple of --eval-interval {args.eval_interval} (offsets are "
                 "staged per evaluation interval: the state is written between two stages)")
    if args.resume is not None and not os.path.isfile(args.resume):
        ap.error(f"--resume: no training state at {args.resume}")
    if args.state_path is None:
        args.state_path = get_model_path(args.model_dir, args.model, args.scale)[:-len(".pt")] + ".state.pt"
    return args


def doc_separator_id(token: Optional[str], encode, vocab_size: int) -> Optional[int]:
    """--doc-separator TOKEN -> token id: an integer id, or a single character looked up in the tokenizer's table (``encode``, None
    when the run has no text to build one from).  SystemExit names a character that is not in the vocabulary."""
    if token is None:
        return None
    try:
        tid = int(token)
    except ValueError:
        if len(token) != 1:
            raise SystemExit(f"--doc-separator: {token!r} is neither an integer token id nor a single character") from None
        if encode is None:
            raise SystemExit(f"--doc-separator: the character {token!r} needs the tokenizer's table (--data)") from None
        try:
            tid = int(encode(token)[0])
        except KeyError:
            raise SystemExit(f"--doc-separator: the character {token!r} is not in the vocabulary") from None
    if not 0 <= tid < vocab_size:
        raise SystemExit(f"--doc-separator: token id {tid} is outside the vocabulary [0, {vocab_size})")
    return tid


def _to_cpu(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def run_args(args, K: int, world: int) -> dict:
    """the arguments a resumed run must repeat (RUN_ARG_DEFAULTS: those a file written before they existed ran with)"""
    return {"model": args.model, "preset": args.preset, "scale": bool(args.scale), "precision": args.precision, "accum_steps": K,
            "world_size": world, "lr_schedule": args.lr_schedule, "warmup_steps": int(args.warmup_steps), "min_lr": float(args.min_lr),
            "no_decay": list(args.no_decay), "label_smoothing": float(args.label_smoothing), "z_loss": float(args.z_loss),
            "ema_decay": None if args.ema_decay is None else float(args.ema_decay), "ema_warmup": bool(args.ema_warmup),
            # the table's length: the step count the schedule was laid out over
            "schedule_iters": None if args.lr_schedule == "reference" else int(args.iters),
            # (only where set: a run without it writes the file it always wrote; load_run_state compares it in both directions)
            **({} if getattr(args, "ignore_token", None) is None else {"ignore_token": int(args.ignore_token)})}


RUN_ARG_DEFAULTS = {"lr_schedule": "reference", "warmup_steps": 0, "min_lr": 0.0, "no_decay": [], "schedule_iters": None,
                    "label_smoothing": 0.0, "z_loss": 0.0, "ema_decay": None, "ema_warmup": False}


def save_run_state(path: str, *, next_iteration: int, sched_steps: int, must_match: dict, model, engine=None, optimizer=None,
                   rank: int = 0, world: int = 1) -> None:
    """the harness's training state: the engine's state_dict() (autograd path: the model's and optim.AdamW's) and, beside it, the
    next iteration, the scheduler's count, the global CPU generator and the must-match arguments.  Refuses a diverged run
    (RuntimeError; the file already there stays as it is).  Rank 0 writes; every rank waits for it."""
    if not (engine if engine is not None else optimizer).is_finite():
        raise RuntimeError(f"refusing to save a diverged run: weights or Adam moments are not finite after iteration {next_iteration}; "
                           f"{path} is left as it was")
    if rank == 0:
        obj = {"format": CK.FORMAT, "version": CK.VERSION, "iteration": int(next_iteration), "sched_steps": int(sched_steps),
               "rng_state": torch.get_rng_state(), "args": dict(must_match),
               "engine": engine.state_dict() if engine is not None else None,
               "model": None if engine is not None else {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
               "optimizer": None if engine is not None else _to_cpu(optimizer.state_dict())}
        CK.save_train_state(path, obj)
    if world > 1:
        torch.distributed.barrier()


def load_run_state(path: str, must_match: dict) -> dict:
    """read and check a file written by save_run_state; SystemExit names the first argument that differs"""
    try:
        st = CK.load_train_state(path)
        for k in ("iteration", "sched_steps", "rng_state", "args", "engine", "model", "optimizer"):
            if k not in st:
                raise ValueError(f"training state {path}: missing key {k!r}")
    except ValueError as e:
        raise SystemExit(f"--resume: {e}") from None
    for field, own in must_match.items():
        saved = st["args"].get(field, RUN_ARG_DEFAULTS.get(field, "<absent>"))
        if saved != own:
            raise SystemExit(f"--resume: {field} differs: {path} was written with {saved!r}, this run has {own!r}")
    saved, own = st["args"].get("ignore_token"), must_match.get("ignore_token")
    if saved != own:
        raise SystemExit(f"--resume: ignore_token differs: {path} was written with {saved!r}, this run has {own!r}")
    return st


def main(argv=None):
    args = parse_args(argv)
    K = check_accum_steps(args.accum_steps)

    torch.manual_seed(42)
    if not torch.cuda.is_available():
        raise SystemExit("drakegpt_amd.train needs an MI355X (no CPU path)")
    rank, local_rank, world = ddist.env_world()
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    pg = ddist.init("nccl", device)

    if bool(args.train_data) != bool(args.val_data):
        raise SystemExit("--train-data and --val-data go together")
    decode = lambda ids: " ".join(str(i) for i in ids)      # noqa: E731
    encode = None                                           # the tokenizer's table, where the run has a text
    if args.train_data:
        # the reference's flow (src/train.py:94-100): token streams from the .pt files, the mapper from the text
        train_data, val_data = load_train_val_data(args.train_data, args.val_data)
        if args.data:
            with open(args.data, "r", encoding="utf-8") as f:
                encode, decode, vocab_size = get_mapper(f.read())
        else:
            vocab_size = int(max(train_data.max(), val_data.max())) + 1
    elif args.data:
        with open(args.data, "r", encoding="utf-8") as f:
            text = f.read()
        data, decode, vocab_size = encode_text(text)
        encode = get_mapper(text)[0]
        train_data, val_data = split_train_val(data)
    else:
        vocab_size = DRAKE_VOCAB_SIZE
        data = torch.randint(0, vocab_size, (1_000_000,), generator=torch.Generator().manual_seed(42))
        train_data, val_data = split_train_val(data)
    train_dev, val_dev = train_data.to(device), val_data.to(device)

    params = PRESETS[args.preset] if args.preset else (SCALE_PARAMS if args.scale else PARAMS)
    vocab_size = params.get("vocab_size", vocab_size)
    doc_sep = doc_separator_id(args.doc_separator, encode, vocab_size)
    model, model_config, params = build_model(args.model, False, params, params, vocab_size, device, args.precision)
    if rank == 0:
        print(f"Selected {args.model} model for training. Model has {model_params(params, args.model, vocab_size)} parameters "
              f"(reference estimate; actual {sum(p.numel() for p in model.parameters())})."
              + ("" if doc_sep is None else f" Document separator: token {doc_sep} (no attention across it)."))
    if doc_sep is not None:
        model.set_doc_separator(doc_sep)          # forward(idx, targets) in train() and eval(); the engine below gets it as well
    B, T = params["batch_size"], params["context_length"]
    base_lr, max_lr = params["base_lr"], params["max_lr"]

    table = lr_values(args, base_lr, max_lr)          # one rate per optimizer step, or None: the reference's CyclicLR at evaluations

    # the update guard's two options: nothing for a run without the flags, whose constructors get the arguments they always got
    guard_kw = {"skip_nonfinite": True, "skip_grad_norm": args.skip_grad_norm} if args.skip_nonfinite else {}
    engine = None
    if args.model == "TransformerLM":
        from .engine import TrainEngine
        engine = TrainEngine(model, B, T, lr=base_lr, betas=params["betas"], seed=42, rank=rank, world_size=world, process_group=pg,
                             max_grad_norm=args.grad_clip, accum_steps=K, lr_schedule=table, no_decay=args.no_decay,
                             label_smoothing=args.label_smoothing, z_loss=args.z_loss,
                             **({} if args.ignore_token is None else {"ignore_index": args.ignore_token}),
                             **({} if doc_sep is None else {"doc_separator": doc_sep}),
                             **guard_kw,
                             **({} if args.ema_decay is None else {"ema_decay": args.ema_decay, "ema_warmup": args.ema_warmup}))
        engine.set_corpus(train_dev)
    else:
        # the five earlier-stage models train through the autograd path; their flat-buffer AdamW all-reduces the gradient
        from .optim import AdamW
        # (smoothing / z-loss in train() mode only: evaluate_loss runs in eval(); the ignored token in both)
        model.set_loss_options(args.label_smoothing, args.z_loss, **({} if args.ignore_token is None else {"ignore_index": args.ignore_token}))
        groups = model.parameters()
        if args.no_decay:
            groups = no_decay_groups(model, args.no_decay)
        optimizer = AdamW(groups, lr=base_lr, betas=params["betas"], process_group=pg, world_size=world,
                          max_grad_norm=args.grad_clip, **guard_kw,
                          **({} if args.ema_decay is None else {"ema_decay": args.ema_decay, "ema_warmup": args.ema_warmup}))
        if table is not None:
            table = schedules.as_table(table).tolist()          # the fp32 values the engine's table would hold

    must_match = run_args(args, K, world)
    start = 0
    sched = {"steps": 0}
    if args.resume:
        st = load_run_state(args.resume, must_match)
        if (st["engine"] is None) != (engine is None):
            raise SystemExit(f"--resume: {args.resume} does not hold the state of a {args.model} run")
        try:
            if engine is not None:
                engine.load_state_dict(st["engine"])
            else:
                model.load_state_dict(st["model"])
                optimizer.load_state_dict(st["optimizer"])
        except ValueError as e:
            raise SystemExit(f"--resume: {e}") from None
        start, sched["steps"] = int(st["iteration"]), int(st["sched_steps"])
        if start > args.iters:
            raise SystemExit(f"--resume: {args.resume} is at iteration {start}, past --iters {args.iters}")
        torch.set_rng_state(st["rng_state"])          # the generator that draws offsets, evaluation batches and the sample
        if rank == 0:
            print(f"resumed {args.resume} at iteration {start}")

    def check_skips(it):
        """the guard's run of skipped updates, read where the host has synchronised anyway: a gradient that never recovers ends the
        run instead of idling through the remaining iterations"""
        n = (engine if engine is not None else optimizer).consecutive_skips()
        if n > args.max_consecutive_skips:
            raise RuntimeError(f"the update guard skipped {n} optimizer updates in a row up to iteration {it} (--max-consecutive-skips "
                               f"{args.max_consecutive_skips}): the gradient does not recover")

    def save_state(next_it):
        if args.skip_nonfinite:
            check_skips(next_it)
        save_run_state(args.state_path, next_iteration=next_it, sched_steps=sched["steps"], must_match=must_match, model=model,
                       engine=engine, optimizer=None if engine is not None else optimizer, rank=rank, world=world)

    averaged = (engine if engine is not None else optimizer).ema_weights if args.ema_decay is not None else None

    model.train()
    t0 = time.perf_counter()

    def on_eval(it):
        model.eval()
        if engine is not None:
            # the evaluation synchronises the host for its losses anyway: the one place inside the loop where reading the
            # grouped dW GEMM's sticky error word costs nothing.  Raises (-> non-zero exit) if a hand-over ever timed out:
            # every weight gradient since then is suspect, and the losses would still look plausible.
            engine.check_status()
        drawn = {}
        losses = evaluate_loss(train_dev, val_dev, model, args.eval_iters, T, B, device, engine=engine, drawn=drawn)
        if averaged is not None:
            # the averaged weights on val_loss's own batches: nothing more is drawn from the host generator, so the run's
            # train_loss / val_loss / lr are those of the run without --ema-decay
            with averaged():
                losses["val_ema"] = evaluate_loss(train_dev, val_dev, model, args.eval_iters, T, B, device, engine=engine,
                                                  offsets={"val": drawn["val"]})["val"]
        if args.skip_nonfinite:
            check_skips(it + 1)
        sched["steps"] += 1
        if table is not None:
            # a per-step schedule: nothing to set here; report the rate of the next step
            lr = engine.current_lr() if engine is not None else table[min(it + 1, len(table) - 1)]
        else:
            lr = cyclic_lr(sched["steps"], base_lr, max_lr)
            if engine is not None:
                engine.set_lr(lr)
            else:
                for g in optimizer.param_groups:
                    g["lr"] = lr
        if rank == 0:
            el = time.perf_counter() - t0
            line = {"step": it + 1, "train_loss": float(losses["train"]), "val_loss": float(losses["val"]), "lr": lr,
                    "tokens_per_s": (it + 1 - start) * K * B * T * world / el}
            if averaged is not None:
                line["val_loss_ema"] = float(losses["val_ema"])
            if args.grad_clip is not None:
                # the last step's pre-clip norm: the evaluation has synchronised the stream already
                line["grad_norm"] = float((engine if engine is not None else optimizer).last_grad_norm)
            if args.skip_nonfinite:
                line["skipped"] = (engine if engine is not None else optimizer).skipped_steps()
            print(json.dumps(line), flush=True)
        model.train()
        if args.save_every and (it + 1) % args.save_every == 0:
            save_state(it + 1)

    if engine is not None:
        engine_loop(engine, len(train_data), T, B, rank, world, args.iters, args.eval_interval, on_eval, device, accum_steps=K,
                    start=start)
    else:
        from . import ops
        for it in range(start, args.iters):
            if table is not None:
                for g in optimizer.param_groups:
                    g["lr"] = table[min(it, len(table) - 1)]
            if K == 1:
                ix = ddist.shard_rows(draw_offsets(len(train_data), T, B * world, None), rank, world).to(device, non_blocking=True)
                x, y = ops.batch_gather(train_dev, ix, T)
                logits, loss = model(x, y)
                optimizer.zero_grad()
                loss.backward()
            else:
                # K micro-batches per step: autograd sums (loss / K).backward() into .grad -- the mean gradient over all K
                optimizer.zero_grad()
                for _ in range(K):
                    ix = ddist.shard_rows(draw_offsets(len(train_data), T, B * world, None), rank, world).to(device, non_blocking=True)
                    x, y = ops.batch_gather(train_dev, ix, T)
                    logits, loss = model(x, y)
                    (loss / K).backward()
            optimizer.step()
            if (it + 1) % args.eval_interval == 0:
                on_eval(it)

    if args.save_every and args.iters % args.save_every:
        save_state(args.iters)      # before the sample is drawn: a longer run continued from here sees the uninterrupted run's generator
    model.eval()
    if rank == 0:
        idx = torch.zeros((1, 1), dtype=torch.long, device=device)
        sample_kw = {}
        if (args.sampler, args.temperature, args.top_k, args.top_p, args.min_p) != ("host", 1.0, None, None, None):
            sample_kw = dict(sampler=args.sampler, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, min_p=args.min_p)
        if (args.repetition_penalty, args.presence_penalty, args.frequency_penalty, args.stop_token) != (1.0, 0.0, 0.0, None):
            sample_kw.update(repetition_penalty=args.repetition_penalty, presence_penalty=args.presence_penalty,
                             frequency_penalty=args.frequency_penalty, stop_tokens=args.stop_token)
        path = get_model_path(args.model_dir, args.model, args.scale)
        # --ema-decay: the sample comes from the averaged weights, which are saved beside the raw checkpoint in its format
        with (averaged() if averaged is not None else contextlib.nullcontext()):
            if args.sample_logprobs or args.top_logprobs or args.best_of > 1:
                if args.best_of > 1 and not args.stop_token:
                    sample_kw["pad_token"] = 0
                gen = model.generate(idx, max_new_tokens=args.sample, return_logprobs=True, top_logprobs=args.top_logprobs,
                                     best_of=args.best_of, **sample_kw)
                n = int(gen.lengths[0])
                print(decode(gen.ids[0, :n].tolist()))
                mean = float(gen.logprobs[0, 1:n].double().mean()) if n > 1 else float("nan")
                line = f"sample logprob: mean {mean:.4f}, perplexity {math.exp(-mean):.3f} over {n - 1} tokens"
                if args.top_logprobs:
                    line += f", top-1 {float((gen.top_ids[0, 1:n, 0] == gen.ids[0, 1:n]).double().mean()):.3f}"
                if args.best_of > 1:
                    line += f", best of {args.best_of}"
                print(line)
            else:
                print(decode(model.generate(idx, max_new_tokens=args.sample, **sample_kw)[0].tolist()))
            if averaged is not None and not args.no_save:
                os.makedirs(args.model_dir, exist_ok=True)
                ema_path = path[:-len(".pt")] + ".ema.pt"
                torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, ema_path)
                print(f"saved {ema_path}")
        if not args.no_save:
            os.makedirs(args.model_dir, exist_ok=True)
            torch.save({k: v.detach().cpu().clone() for k, v in model.state_dict().items()}, path)
            print(f"saved {path}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
