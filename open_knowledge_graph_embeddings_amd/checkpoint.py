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

ENTITY_KEY, RELATION_KEY = "entity_embedding.weight", "relation_embedding.weight"


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


def _frozen(step):
    """None, or the table a FusedTrainStep(freeze=...) does not train: "entities" / "relations" """
    return getattr(step, "freeze", None)


def freeze_names(freeze_param, loaded):
    """the reference's `freeze_param` (Trainer.load_state_dict, trainer.py:532-536): a list of parameter names, or ["True"] for
    every loaded name -> the names of `loaded` to freeze.  None / not a list / empty: none"""
    if type(freeze_param) is not list or not freeze_param:
        return []
    if type(freeze_param[0]) is str and freeze_param[0] == "True":
        return list(loaded)
    return [name for name in loaded if name in freeze_param]


def _full_tables(step):
    """(E, R, sumE, sumR) as full tables, whatever the step class; an Adam step: (E, R, mE, vE, mR, vR).  A frozen table's
    missing state comes as None."""
    if _is_adam(step):
        return step.E, step.R, step.mE, step.vE, step.mR, step.vR
    if hasattr(step, "flush"):                                    # deferred weight decay: rows may owe decay-only steps
        step.flush()
    if hasattr(step, "ent_lo"):                                   # ShardedTrainStep: gather the row shards
        return (_gather_rows(step.E, step.n_ent, step.group), step.R, _gather_rows(step.sumE, step.n_ent, step.group),
                step.sumR)
    return step.E, step.R, step.sumE, step.sumR


def to_reference_checkpoint(step, epoch=0, training_steps=None):
    """The dict `Trainer.save` would write for this training state (tensors on the CPU).  An Adam step (FusedTrainStep(optimizer=
    "adam")) writes torch.optim.Adam's layout -- state {step, exp_avg, exp_avg_sq}, `step` = the optimizer steps taken, regime
    optimizer "Adam" -- which torch.optim.Adam.load_state_dict takes as it is."""
    if _is_adam(step):
        return _adam_checkpoint(step, epoch, training_steps)
    E, R, sumE, sumR = (None if t is None else t.detach().cpu().clone() for t in _full_tables(step))
    n_steps = float(step.steps)
    # a frozen table (FusedTrainStep(freeze=...)): the `sum` the step holds for it, untouched -- zeros where it never had one,
    # torch.optim.Adagrad's initial state -- and the step count of a parameter that never had a gradient
    steps_e, steps_r = (0.0 if _frozen(step) == "entities" else n_steps), (0.0 if _frozen(step) == "relations" else n_steps)
    sumE, sumR = (torch.zeros_like(E) if sumE is None else sumE), (torch.zeros_like(R) if sumR is None else sumR)
    group = {"lr": step.lr, "betas": (0.9, 0.999), "eps": step.eps, "weight_decay": step.weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": False, "lr_decay": 0, "initial_accumulator_value": 0, "params": [0, 1]}
    optimizer_state = {"state": {0: {"step": torch.tensor(steps_e), "sum": sumE},
                                 1: {"step": torch.tensor(steps_r), "sum": sumR}},
                       "param_groups": [group]}
    regime = [{"optimizer": "Adagrad", "epoch": 0, "lr": step.lr, "weight_decay": step.weight_decay}]
    return {"epoch": int(epoch), "training_steps": int(step.steps if training_steps is None else training_steps),
            "state_dict": {ENTITY_KEY: E, RELATION_KEY: R},
            "optimizer_state_dict": [{"optimizer_state": optimizer_state, "regime": regime}],
            "validation_results": None}


def _adam_checkpoint(step, epoch, training_steps):
    E, R, mE, vE, mR, vR = (None if t is None else t.detach().cpu().clone() for t in _full_tables(step))
    t = float(step.adam_t)
    group = {"lr": step.lr, "betas": tuple(step.betas), "eps": step.eps, "weight_decay": step.weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": False, "params": [0, 1]}
    optimizer_state = {"state": {0: {"step": torch.tensor(t), "exp_avg": mE, "exp_avg_sq": vE},
                                 1: {"step": torch.tensor(t), "exp_avg": mR, "exp_avg_sq": vR}},
                       "param_groups": [group]}
    if _frozen(step) is not None:     # torch.optim.Adam creates a parameter's state at its first step: a frozen one has no entry
        del optimizer_state["state"][0 if _frozen(step) == "entities" else 1]
    regime = [{"optimizer": "Adam", "epoch": 0, "lr": step.lr, "weight_decay": step.weight_decay}]
    return {"epoch": int(epoch), "training_steps": int(step.steps if training_steps is None else training_steps),
            "state_dict": {ENTITY_KEY: E, RELATION_KEY: R},
            "optimizer_state_dict": [{"optimizer_state": optimizer_state, "regime": regime}],
            "validation_results": None}


def _checkpoint_optimizer(ckpt):
    """'adam' / 'adagrad': what the state entries of the first parameter say (the regime's name where there is no state yet)"""
    reg = ckpt["optimizer_state_dict"][0]
    states = reg["optimizer_state"]["state"]
    st0 = states.get(0) or states.get(1, {})            # (an Adam run with the entity table frozen holds no entry 0)
    if "exp_avg" in st0:
        return "adam"
    if "sum" in st0:
        return "adagrad"
    names = [str(r.get("optimizer", "")).lower() for r in reg.get("regime", []) if isinstance(r, dict)]
    return "adam" if names and names[-1].endswith("adam") else "adagrad"


def save_checkpoint(path, step, epoch=0, training_steps=None):
    """Collective for the sharded step (every rank calls it); rank 0 writes."""
    ckpt = to_reference_checkpoint(step, epoch, training_steps)
    if not hasattr(step, "ent_lo") or step.rank == 0:
        torch.save(ckpt, path)
    return ckpt


def load_reference_checkpoint(step, ckpt_or_path, reset_optimizer=False, freeze_param=None):
    """Load tables (and, unless `reset_optimizer`, the Adagrad accumulators and step count -- the reference's
    `Trainer.load(reset_optimizer=...)` switch, trainer.py:561-605) into a fused / sharded train step.
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
    if not reset_optimizer:
        want, have = ("adam" if _is_adam(step) else "adagrad"), _checkpoint_optimizer(ckpt)
        if want != have:
            raise ValueError(f"the checkpoint holds {have} optimizer state and this step trains with {want}: its accumulators do "
                             f"not carry over -- load with reset_optimizer=True to take the tables alone")
    if names:                                                     # (every refusal is behind us)
        step.set_freeze("entities" if names[0] == ENTITY_KEY else "relations")
    if hasattr(step, "flush"):                                    # deferred weight decay: no row may owe steps to the loaded tables
        step.flush()
    step.E.copy_(E[lo:hi])
    step.R.copy_(R)
    if _is_adam(step):
        _load_adam_state(step, None if reset_optimizer else ckpt["optimizer_state_dict"][0]["optimizer_state"], ckpt)
    elif reset_optimizer:
        for s in (step.sumE, step.sumR):
            if s is not None:
                s.zero_()
        step.steps = 0
    else:
        st = ckpt["optimizer_state_dict"][0]["optimizer_state"]
        group, state = st["param_groups"][0], st["state"]
        if _frozen(step) is not None:
            # the frozen table's `sum` is carried along untouched; the step count is the trained table's
            for name, idx, table in (("sumE", 0, step.E), ("sumR", 1, step.R)):
                if getattr(step, name) is None:
                    setattr(step, name, torch.empty_like(table))
                getattr(step, name).copy_(state[idx]["sum"])
            step.steps = int(float(state[1 if _frozen(step) == "entities" else 0]["step"]))
        else:
            step.sumE.copy_(state[0]["sum"][lo:hi])
            step.sumR.copy_(state[1]["sum"])
            # (the larger count: a file written by a frozen run holds `step` 0 for the table that never had a gradient, and the
            #  dropout masks are keyed by the step count)
            step.steps = int(max(float(state[0]["step"]), float(state[1]["step"])))
        step.lr, step.weight_decay, step.eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
        if float(group.get("lr_decay", 0)) != 0 or float(group.get("initial_accumulator_value", 0)) != 0:
            raise NotImplementedError("Adagrad lr_decay / initial_accumulator_value are not used by the reference configs")
    for g in (step.dE, step.dR):                                  # (the row-sparse step keeps no dense gradients, a frozen table none)
        if g is not None:
            g.zero_()
    return ckpt


def _load_adam_state(step, st, ckpt):
    """moments, t and hyper-parameters of an Adam step from torch.optim.Adam's state (None: reset -- zero moments, t = 0)"""
    trained = [i for i, name in ((0, "entities"), (1, "relations")) if _frozen(step) != name]      # (a frozen table has no state)
    if st is None or trained[0] not in st["state"]:              # (a torch optimizer that has not stepped yet holds no state)
        for x in (step.mE, step.vE, step.mR, step.vR):
            if x is not None:
                x.zero_()
        step.set_adam_t(0)
        step.steps = 0
        return
    group, state = st["param_groups"][0], st["state"]
    if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
        raise NotImplementedError("amsgrad, maximize and decoupled weight decay (AdamW) are not implemented")
    if 0 in trained:
        step.mE.copy_(state[0]["exp_avg"])
        step.vE.copy_(state[0]["exp_avg_sq"])
    if 1 in trained:
        step.mR.copy_(state[1]["exp_avg"])
        step.vR.copy_(state[1]["exp_avg_sq"])
    step.set_adam_t(int(float(state[trained[0]]["step"])))
    step.steps = int(ckpt.get("training_steps", int(float(state[trained[0]]["step"]))))
    step.lr, step.weight_decay, step.eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
    step.betas = (float(group["betas"][0]), float(group["betas"][1]))


# ------------------------------------------------------------------------------------------------------------------
# The token-encoded and Tucker3 models: a module and the driver its train_step() returned
# ------------------------------------------------------------------------------------------------------------------
CHECKPOINT_FORMAT = 1
_OPTIMIZER_MISMATCH = ("the checkpoint holds {have} optimizer state and this step trains with {want}: its accumulators do "
                       "not carry over -- load with reset_optimizer=True to take the tables alone")


def _model_and_step(model, step):
    from .step_optim import StepOptimizer
    if not isinstance(step, StepOptimizer) or not hasattr(model, "optimizer_params_and_state"):
        raise TypeError(f"model_checkpoint / load_model_checkpoint take a token-encoded or Tucker3 model and the driver its "
                        f"train_step() returned, not {type(step).__name__}: the two-table lookup steps go through "
                        f"to_reference_checkpoint / load_reference_checkpoint")
    return model.optimizer_params_and_state(step)


def _state_names(step):
    return ("exp_avg", "exp_avg_sq") if _is_adam(step) else ("sum",)


def model_checkpoint(model, step, epoch=0, training_steps=None):
    """The dict `Trainer.save` would write for `model` trained by `step` (= model.train_step(...)), tensors on the CPU:
    state_dict = the module's own (integer buffers as int64, the reference's token-id dtype), taken once the step has settled its
    deferred updates and brought the module's batch-norm modules up to date; optimizer_state = what torch.optim.Adagrad /
    torch.optim.Adam over model.parameters() would return from state_dict(), every entry a copy in its parameter's shape; and one
    extra top-level key "okge" (Trainer.save appends its save_info the same way): plain numbers a resumed run needs to draw the
    same dropout masks and that torch's optimizer state has no place for."""
    entries, word = _model_and_step(model, step)
    step.sync_module()
    cpu = lambda t: t.detach().cpu().clone()                   # noqa: E731
    state_dict = {k: cpu(v) if v.is_floating_point() else cpu(v).to(torch.int64) for k, v in model.state_dict().items()}
    adam = _is_adam(step)
    t = float(int(word[0].item())) if adam else float(step.steps)
    state = {}
    for i, (p, views, moved) in enumerate(entries):
        if adam and not moved:                                  # torch.optim.Adam creates a parameter's state at its first step
            continue
        state[i] = {"step": torch.tensor(t if moved else 0.0)}
        state[i].update({name: cpu(v) for name, v in zip(_state_names(step), views)})
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
            "validation_results": None,
            "okge": {"format": CHECKPOINT_FORMAT, "steps": int(step.steps), "dropout_step": int(model.dropout_step),
                     "dropout_seed": int(model.dropout_seed), "grad_clip": float(step.grad_clip)}}


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
    if reset_optimizer:
        return
    want, have = ("adam" if _is_adam(step) else "adagrad"), _checkpoint_optimizer(ckpt)
    if want != have:
        raise ValueError(_OPTIMIZER_MISMATCH.format(have=have, want=want))
    st = ckpt["optimizer_state_dict"][0]["optimizer_state"]
    group, state = st["param_groups"][0], st["state"]
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
    st = None if reset_optimizer else ckpt["optimizer_state_dict"][0]["optimizer_state"]
    state = {} if st is None else st["state"]
    for i, (p, views, moved) in enumerate(entries):
        for name, v in zip(_state_names(step), views):
            if i in state:
                v.copy_(state[i][name])
            else:                                                # (reset, or a parameter torch's Adam has not stepped yet)
                v.zero_()
    taken = [int(float(state[i]["step"])) for i, e in enumerate(entries) if e[2] and i in state]
    if _is_adam(step):
        step.set_adam_t(taken[0] if taken else 0)
    if st is None:
        step.steps = 0
        return ckpt
    group = st["param_groups"][0]
    step.lr, step.weight_decay, step.eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
    if _is_adam(step):
        step.betas = (float(group["betas"][0]), float(group["betas"][1]))
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
