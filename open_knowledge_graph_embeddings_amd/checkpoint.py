"""Checkpoint interop with the reference: `Trainer.save` / `Trainer.load`
(openkge/trainer.py:561-638) store

    {"epoch", "training_steps", "state_dict": model.state_dict(),
     "optimizer_state_dict": [OptimRegime.state_dict(), ...], "validation_results", "results"}

with model keys `entity_embedding.weight` / `relation_embedding.weight` and, per OptimRegime
(utils/optim.py:170-193), {"optimizer_state": torch.optim.Adagrad.state_dict(), "regime": [config...]}: Adagrad
state `{param index: {"step": float tensor, "sum": tensor}}`, parameter 0 = entity table, 1 = relation table, and one
param group that still carries the keys of the Adam shell the regime was born as (betas, amsgrad, eps=1e-8 ...).

These functions move that layout to and from the fused train steps (tables, Adagrad accumulators, step counter), for
one device or for the row-sharded step (shards are gathered to / scattered from full tables).  A FusedTrainStep(optimizer="adam")
writes and reads torch.optim.Adam's state instead ({"step", "exp_avg", "exp_avg_sq"}, regime optimizer "Adam"); Adagrad state
is refused by an Adam step and the other way round unless `reset_optimizer` is set.  Files written here
contain tensors and plain containers only, so they load with `torch.load(..., weights_only=True)`; the reference's own
`results` entry (a pickled ResultsLog object) is never written and never read.

The models whose rows are encoded from tokens, the Tucker3 model and the lookup models with an `_encode` variant on
(lookup_variants.LookupVariantTrainStep) train more than two tensors: model_checkpoint /
save_model_checkpoint / load_model_checkpoint (below) move the same layout -- the module's whole state_dict, one optimizer state
entry per parameter in model.parameters() order -- between a module and the driver its train_step() returned.  Which part of
which buffer of the step belongs to which parameter is the embedders' knowledge (optimizer_params_and_state); nothing else of
a step's optimizer state is read here.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from .train_step import ENTITY_KEY, RELATION_KEY

CHECKPOINT_FORMAT = 1


def _gather_rows(local, n_rows, group):
    """all ranks' row blocks -> full (n_rows, d) tensor on every rank (blocks padded to the largest)."""
    world = dist.get_world_size(group)
    per = (n_rows + world - 1) // world
    pad = torch.zeros((per, local.shape[1]), dtype=local.dtype, device=local.device)
    pad[:local.shape[0]] = local
    out = torch.empty((world * per, local.shape[1]), dtype=local.dtype, device=local.device)
    dist.all_gather_into_tensor(out.view(-1), pad.view(-1), group=group)
    return out[:n_rows]


def _is_adam(step):
    return getattr(step, "optimizer", "adagrad") == "adam"


def _state_names(step):
    return ("exp_avg", "exp_avg_sq") if _is_adam(step) else ("sum",)


def _cpu(t):
    return t.detach().cpu().clone()


def freeze_names(freeze_param, loaded):
    """the reference's `freeze_param` (Trainer.load_state_dict, trainer.py:532-536): a list of parameter names, or ["True"] for
    every loaded name -> the names of `loaded` to freeze.  None / not a list / empty: none"""
    if type(freeze_param) is not list or not freeze_param:
        return []
    if type(freeze_param[0]) is str and freeze_param[0] == "True":
        return list(loaded)
    return [name for name in loaded if name in freeze_param]


def _lookup_entries(step, full=False, keep_sums=False):
    """{state_dict key: (parameter, its optimizer state tensors, moved)} of a two-table lookup step -- what
    optimizer_params_and_state gives for the steps of the other models -- in the order of the reference's optimizer: the entity
    table, the relation table.  moved: the step trains the table (FusedTrainStep(freeze=...) does not train one); a state tensor
    the step does not hold comes as None.  The one place that knows a lookup step by its attribute names: FusedTrainStep, the
    row-sharded step and a bare object with the tables and accumulators all serve.
    full: the row shards of a ShardedTrainStep gathered into whole tables (collective).  keep_sums: an Adagrad step gets a `sum`
    where it holds none (a frozen table carries the file's along untouched)."""
    names = (("mE", "vE"), ("mR", "vR")) if _is_adam(step) else (("sumE",), ("sumR",))
    entries = {}
    for key, table, letter, state in ((ENTITY_KEY, "entities", "E", names[0]), (RELATION_KEY, "relations", "R", names[1])):
        p = getattr(step, letter)
        if keep_sums and not _is_adam(step) and getattr(step, state[0], None) is None:
            setattr(step, state[0], torch.empty_like(p))
        views = tuple(getattr(step, name, None) for name in state)
        if full and letter == "E" and hasattr(step, "ent_lo"):
            p, *views = (_gather_rows(t, step.n_ent, step.group) for t in (p, *views))
        entries[key] = (p, tuple(views), getattr(step, "freeze", None) != table)
    return entries


def _reference_checkpoint(step, state_dict, entries, t, epoch, training_steps):
    """The dict `Trainer.save` writes around `state_dict`: what torch.optim.Adagrad / torch.optim.Adam over the parameters of
    `entries` ([(parameter, state tensors, moved)]) would return from state_dict(), every tensor a copy on the CPU, and the regime.
    t: the optimizer steps taken.  Adagrad holds state for every parameter from its construction: one that is not moved has
    `step` 0 and the `sum` the step holds for it -- zeros where it holds none; Adam creates a parameter's state at its first step:
    one that is not moved has no entry."""
    adam = _is_adam(step)
    state = {}
    for i, (p, views, moved) in enumerate(entries):
        if adam and not moved:
            continue
        state[i] = {"step": torch.tensor(t if moved else 0.0)}
        state[i].update({name: torch.zeros_like(_cpu(p)) if v is None else _cpu(v) for name, v in zip(_state_names(step), views)})
    group = {"lr": step.lr, "betas": tuple(step.betas) if adam else (0.9, 0.999), "eps": step.eps, "weight_decay": step.weight_decay,
             "amsgrad": False, "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": False}
    if not adam:
        group.update({"lr_decay": 0, "initial_accumulator_value": 0})
    group["params"] = list(range(len(entries)))
    regime = [{"optimizer": "Adam" if adam else "Adagrad", "epoch": 0, "lr": step.lr, "weight_decay": step.weight_decay}]
    return {"epoch": int(epoch), "training_steps": int(step.steps if training_steps is None else training_steps),
            "state_dict": state_dict,
            "optimizer_state_dict": [{"optimizer_state": {"state": state, "param_groups": [group]}, "regime": regime}],
            "validation_results": None}


def to_reference_checkpoint(step, epoch=0, training_steps=None):
    """The dict `Trainer.save` would write for this training state (tensors on the CPU).  An Adam step (FusedTrainStep(optimizer=
    "adam")) writes torch.optim.Adam's layout -- state {step, exp_avg, exp_avg_sq}, `step` = the optimizer steps taken, regime
    optimizer "Adam" -- which torch.optim.Adam.load_state_dict takes as it is."""
    if hasattr(step, "flush"):                                    # deferred weight decay: rows may owe decay-only steps
        step.flush()
    entries = _lookup_entries(step, full=True)
    return _reference_checkpoint(step, {key: _cpu(e[0]) for key, e in entries.items()}, list(entries.values()),
                                 float(step.adam_t if _is_adam(step) else step.steps), epoch, training_steps)


def _checkpoint_optimizer(reg):
    """'adam' / 'adagrad': what the state entries of the first parameter say (the regime's name where there is no state yet)"""
    states = reg["optimizer_state"]["state"]
    st0 = states.get(0) or states.get(1, {})            # (an Adam run with the entity table frozen holds no entry 0)
    if "exp_avg" in st0:
        return "adam"
    if "sum" in st0:
        return "adagrad"
    names = [str(r.get("optimizer", "")).lower() for r in reg.get("regime", []) if isinstance(r, dict)]
    return "adam" if names and names[-1].endswith("adam") else "adagrad"


def _check_optimizer_state(step, entries, reg):
    """every refusal of the optimizer state `reg` (an entry of a checkpoint's optimizer_state_dict) for the parameters of `entries`,
    before anything is written"""
    want, have = ("adam" if _is_adam(step) else "adagrad"), _checkpoint_optimizer(reg)
    if want != have:
        raise ValueError(f"the checkpoint holds {have} optimizer state and this step trains with {want}: its accumulators do "
                         f"not carry over -- load with reset_optimizer=True to take the tables alone")
    group, state = reg["optimizer_state"]["param_groups"][0], reg["optimizer_state"]["state"]
    if len(group["params"]) != len(entries):
        raise ValueError(f"the checkpoint's optimizer holds {len(group['params'])} parameters, this model has {len(entries)}")
    for i, (p, views, moved) in enumerate(entries):
        for name in _state_names(step) if i in state else ():
            if name not in state[i] or tuple(state[i][name].shape) != tuple(p.shape):
                got = tuple(state[i][name].shape) if name in state[i] else None
                raise ValueError(f"optimizer state {name!r} of parameter {i} has shape {got}, the parameter's is {tuple(p.shape)}")
    if float(group.get("lr_decay", 0)) != 0 or float(group.get("initial_accumulator_value", 0)) != 0:
        raise NotImplementedError("Adagrad lr_decay / initial_accumulator_value are not used by the reference configs")
    if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
        raise NotImplementedError("amsgrad, maximize and decoupled weight decay (AdamW) are not implemented")


def _apply_optimizer_state(step, entries, reg):
    """The state tensors of `entries`, the Adam step count and the step's hyper-parameters from `reg` (checked).  reg None, the
    reset: the state is zeroed, the counts are 0 and the step keeps its own hyper-parameters.  A parameter the file holds no state
    for (torch's Adam has not stepped it yet) gets zeros; a state tensor the step does not hold (None: a frozen table's) is passed
    over.  -> the `step` counts of the moved parameters the file holds state for; None after a reset"""
    state = {} if reg is None else reg["optimizer_state"]["state"]
    for i, (p, views, moved) in enumerate(entries):
        for name, v in zip(_state_names(step), views):
            if v is not None and i in state:
                v.copy_(state[i][name])
            elif v is not None:
                v.zero_()
    taken = [int(float(state[i]["step"])) for i, e in enumerate(entries) if e[2] and i in state]
    if _is_adam(step):
        step.set_adam_t(taken[0] if taken else 0)
    if reg is None:
        step.steps = 0
        return None
    group = reg["optimizer_state"]["param_groups"][0]
    step.lr, step.weight_decay, step.eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
    if _is_adam(step):
        step.betas = (float(group["betas"][0]), float(group["betas"][1]))
    return taken


def save_checkpoint(path, step, epoch=0, training_steps=None):
    """Collective for the sharded step (every rank calls it); rank 0 writes."""
    ckpt = to_reference_checkpoint(step, epoch, training_steps)
    if not hasattr(step, "ent_lo") or step.rank == 0:
        torch.save(ckpt, path)
    return ckpt


def load_reference_checkpoint(step, ckpt_or_path, reset_optimizer=False, freeze_param=None):
    """Load tables (and, unless `reset_optimizer`, the Adagrad accumulators and step count -- the reference's
    `Trainer.load(reset_optimizer=...)` switch, trainer.py:561-605) into a fused / sharded train step.  Every refusal is raised
    before anything of the step is written.
    freeze_param (the reference's resume_freeze, trainer.py:532-536): a list of parameter names, or ["True"] for every loaded
    one.  `entity_embedding.weight` / `relation_embedding.weight` set the step's `freeze` (FusedTrainStep.set_freeze) before the
    state is loaded; naming both raises ValueError (nothing to train), a step class without `set_freeze` NotImplementedError."""
    ckpt = ckpt_or_path
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt_or_path, map_location="cpu", weights_only=True)
    sd = ckpt["state_dict"]
    E, R = sd[ENTITY_KEY], sd[RELATION_KEY]
    names = freeze_names(freeze_param, (ENTITY_KEY, RELATION_KEY))
    if len(names) == 2:
        raise ValueError(f"freeze_param {freeze_param!r} names both tables of a bare train step: nothing is left to train")
    if names and not hasattr(step, "set_freeze"):
        raise NotImplementedError(f"{type(step).__name__} cannot freeze a table: freeze_param is built for the single-device "
                                  f"FusedTrainStep")
    lo, hi = (step.ent_lo, step.ent_hi) if hasattr(step, "ent_lo") else (0, E.shape[0])
    if E[lo:hi].shape != step.E.shape or R.shape != step.R.shape:
        raise ValueError(f"checkpoint tables {tuple(E.shape)}, {tuple(R.shape)} do not fit this model")
    reg = None if reset_optimizer else ckpt["optimizer_state_dict"][0]
    if reg is not None and hasattr(step, "ent_lo") and 0 in reg["optimizer_state"]["state"]:       # this rank's rows of the entity state
        st = reg["optimizer_state"]
        own = {k: v if k == "step" else v[lo:hi] for k, v in st["state"][0].items()}
        reg = dict(reg, optimizer_state=dict(st, state={**st["state"], 0: own}))
    if reg is not None:
        _check_optimizer_state(step, list(_lookup_entries(step).values()), reg)
    if names:                                                     # (every refusal is behind us)
        step.set_freeze("entities" if names[0] == ENTITY_KEY else "relations")
    entries = list(_lookup_entries(step, keep_sums=reg is not None).values())
    if _is_adam(step) and reg is not None and [e[2] for e in entries].index(True) not in reg["optimizer_state"]["state"]:
        reg = None                                                # (a torch optimizer that has not stepped yet holds no state)
    if hasattr(step, "flush"):                                    # deferred weight decay: no row may owe steps to the loaded tables
        step.flush()
    step.E.copy_(E[lo:hi])
    step.R.copy_(R)
    taken = _apply_optimizer_state(step, entries, reg)
    if taken is not None:
        # Adagrad, the larger count: a file written by a frozen run holds `step` 0 for the table that never had a gradient (and
        # a frozen step takes the trained table's); the dropout masks are keyed by the step count
        step.steps = int(ckpt.get("training_steps", taken[0])) if _is_adam(step) else max(taken)
    for g in (getattr(step, "dE", None), getattr(step, "dR", None)):      # (the row-sparse step keeps no dense gradients, a frozen table none)
        if g is not None:
            g.zero_()
    return ckpt


# ------------------------------------------------------------------------------------------------------------------
# The token-encoded and Tucker3 models: a module and the driver its train_step() returned
# ------------------------------------------------------------------------------------------------------------------
def _model_and_step(model, step):
    from .step_optim import StepOptimizer
    if not isinstance(step, StepOptimizer) or not hasattr(model, "optimizer_params_and_state"):
        raise TypeError(f"model_checkpoint / load_model_checkpoint take a token-encoded or Tucker3 model and the driver its "
                        f"train_step() returned, not {type(step).__name__}: the two-table lookup steps go through "
                        f"to_reference_checkpoint / load_reference_checkpoint")
    return model.optimizer_params_and_state(step)


def model_checkpoint(model, step, epoch=0, training_steps=None):
    """The dict `Trainer.save` would write for `model` trained by `step` (= model.train_step(...)), tensors on the CPU:
    state_dict = the module's own (integer buffers as int64, the reference's token-id dtype), taken once the step has settled its
    deferred updates and brought the module's batch-norm modules up to date; optimizer_state = what torch.optim.Adagrad /
    torch.optim.Adam over model.parameters() would return from state_dict(), every entry a copy in its parameter's shape; and one
    extra top-level key "okge" (Trainer.save appends its save_info the same way): plain numbers a resumed run needs to draw the
    same dropout masks and that torch's optimizer state has no place for."""
    entries, word = _model_and_step(model, step)
    step.sync_module()
    state_dict = {k: _cpu(v) if v.is_floating_point() else _cpu(v).to(torch.int64) for k, v in model.state_dict().items()}
    t = float(int(word[0].item())) if _is_adam(step) else float(step.steps)
    ckpt = _reference_checkpoint(step, state_dict, entries, t, epoch, training_steps)
    ckpt["okge"] = {"format": CHECKPOINT_FORMAT, "steps": int(step.steps), "dropout_step": int(model.dropout_step),
                    "dropout_seed": int(model.dropout_seed), "grad_clip": float(step.grad_clip)}
    return ckpt


def save_model_checkpoint(path, model, step, epoch=0, training_steps=None):
    """model_checkpoint(...) written with torch.save; -> the dict"""
    ckpt = model_checkpoint(model, step, epoch, training_steps)
    torch.save(ckpt, path)
    return ckpt


def _check_model_checkpoint(model, step, entries, ckpt, reset_optimizer):
    """every refusal of load_model_checkpoint, before anything is written"""
    sd, own = ckpt["state_dict"], model.state_dict()
    for k, v in own.items():
        if k not in sd:
            raise ValueError(f"the checkpoint's state_dict has no {k!r}")
        if tuple(sd[k].shape) != tuple(v.shape):
            raise ValueError(f"checkpoint tensor {k!r} has shape {tuple(sd[k].shape)}, the model's has {tuple(v.shape)}")
    for k in sd:
        if k not in own:
            raise ValueError(f"the checkpoint's state_dict holds {k!r}, which this model does not have")
    extra = ckpt.get("okge")
    if extra is not None and int(extra.get("format", 0)) != CHECKPOINT_FORMAT:
        raise ValueError(f"checkpoint 'okge' format {extra.get('format')!r}: this package reads format {CHECKPOINT_FORMAT}")
    if not reset_optimizer:
        _check_optimizer_state(step, entries, ckpt["optimizer_state_dict"][0])


def load_model_checkpoint(model, step, ckpt_or_path, reset_optimizer=False, freeze_param=None):
    """Load what model_checkpoint or the reference's `Trainer.save` wrote into `model` and its driver `step`, so that the next
    step() continues the run.  reset_optimizer (the reference's `Trainer.load(reset_optimizer=...)` switch): the state_dict
    alone is taken; accumulators / moments, the Adam step count and the step counter start from zero, the step keeps its own
    hyper-parameters.  Without the "okge" key (a file the reference wrote) the step counter is the file's training_steps.
    freeze_param (the reference's resume_freeze, trainer.py:532-536; a list of parameter names, or ["True"] for every loaded
    one): with step=None -- a module trained through AddLossModule and a torch / Okge optimizer, which keeps its own state --
    the state_dict is loaded into the module and the named parameters get requires_grad = False, which AddLossModule reads on
    every call.  The fused drivers of the token-encoded, Tucker3 and lookup-variant models train every tensor they hold: a
    driver together with a non-empty freeze_param raises NotImplementedError before anything is written."""
    ckpt = ckpt_or_path
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt_or_path, map_location="cpu", weights_only=True)
    if step is None:
        own = dict(model.named_parameters())
        model.load_state_dict(ckpt["state_dict"])
        for name in freeze_names(freeze_param, [k for k in ckpt["state_dict"] if k in own]):
            own[name].requires_grad = False
        return ckpt
    if freeze_names(freeze_param, list(ckpt["state_dict"])):
        raise NotImplementedError(f"load_model_checkpoint(freeze_param=...): {type(step).__name__} trains every tensor it holds; "
                                  f"frozen parameters are built for the lookup models (FusedTrainStep(freeze=...), or step=None "
                                  f"and AddLossModule)")
    entries, word = _model_and_step(model, step)
    _check_model_checkpoint(model, step, entries, ckpt, reset_optimizer)
    step.flush()                                                 # no row may owe decay-only steps to the loaded tables
    model.load_state_dict(ckpt["state_dict"])
    if getattr(model, "entity_embedding_from_tokens", None) is not None:      # tables precomputed from the tokens: stale now
        model.entity_embedding_from_tokens = model.relations_embedding_from_tokens = None
    step.adopt_module()
    step.reset_gradients()
    taken = _apply_optimizer_state(step, entries, None if reset_optimizer else ckpt["optimizer_state_dict"][0])
    if taken is None:
        return ckpt
    extra = ckpt.get("okge")
    if extra is None:
        step.steps = int(ckpt.get("training_steps", taken[0] if taken else 0))
        return ckpt
    step.steps = int(extra["steps"])
    model.dropout_step, model.dropout_seed = int(extra["dropout_step"]), int(extra["dropout_seed"])
    step.seed = model.dropout_seed
    step.grad_clip = float(extra["grad_clip"])
    if step.grad_clip > 0 and step.grad_norm is None:
        step.grad_norm = torch.zeros(1, dtype=torch.float64, device=step.device)
    return ckpt
