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


def _full_tables(step):
    """(E, R, sumE, sumR) as full tables, whatever the step class; an Adam step: (E, R, mE, vE, mR, vR)."""
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
    E, R, sumE, sumR = (t.detach().cpu().clone() for t in _full_tables(step))
    n_steps = float(step.steps)
    group = {"lr": step.lr, "betas": (0.9, 0.999), "eps": step.eps, "weight_decay": step.weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": False, "lr_decay": 0, "initial_accumulator_value": 0, "params": [0, 1]}
    optimizer_state = {"state": {0: {"step": torch.tensor(n_steps), "sum": sumE},
                                 1: {"step": torch.tensor(n_steps), "sum": sumR}},
                       "param_groups": [group]}
    regime = [{"optimizer": "Adagrad", "epoch": 0, "lr": step.lr, "weight_decay": step.weight_decay}]
    return {"epoch": int(epoch), "training_steps": int(step.steps if training_steps is None else training_steps),
            "state_dict": {ENTITY_KEY: E, RELATION_KEY: R},
            "optimizer_state_dict": [{"optimizer_state": optimizer_state, "regime": regime}],
            "validation_results": None}


def _adam_checkpoint(step, epoch, training_steps):
    E, R, mE, vE, mR, vR = (t.detach().cpu().clone() for t in _full_tables(step))
    t = float(step.adam_t)
    group = {"lr": step.lr, "betas": tuple(step.betas), "eps": step.eps, "weight_decay": step.weight_decay, "amsgrad": False,
             "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "decoupled_weight_decay": False, "params": [0, 1]}
    optimizer_state = {"state": {0: {"step": torch.tensor(t), "exp_avg": mE, "exp_avg_sq": vE},
                                 1: {"step": torch.tensor(t), "exp_avg": mR, "exp_avg_sq": vR}},
                       "param_groups": [group]}
    regime = [{"optimizer": "Adam", "epoch": 0, "lr": step.lr, "weight_decay": step.weight_decay}]
    return {"epoch": int(epoch), "training_steps": int(step.steps if training_steps is None else training_steps),
            "state_dict": {ENTITY_KEY: E, RELATION_KEY: R},
            "optimizer_state_dict": [{"optimizer_state": optimizer_state, "regime": regime}],
            "validation_results": None}


def _checkpoint_optimizer(ckpt):
    """'adam' / 'adagrad': what the state entries of the first parameter say (the regime's name where there is no state yet)"""
    reg = ckpt["optimizer_state_dict"][0]
    st0 = reg["optimizer_state"]["state"].get(0, {})
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


def load_reference_checkpoint(step, ckpt_or_path, reset_optimizer=False):
    """Load tables (and, unless `reset_optimizer`, the Adagrad accumulators and step count -- the reference's
    `Trainer.load(reset_optimizer=...)` switch, trainer.py:561-605) into a fused / sharded train step."""
    ckpt = ckpt_or_path
    if not isinstance(ckpt, dict):
        ckpt = torch.load(ckpt_or_path, map_location="cpu", weights_only=True)
    sd = ckpt["state_dict"]
    E, R = sd[ENTITY_KEY], sd[RELATION_KEY]
    lo, hi = (step.ent_lo, step.ent_hi) if hasattr(step, "ent_lo") else (0, E.shape[0])
    if E[lo:hi].shape != step.E.shape or R.shape != step.R.shape:
        raise ValueError(f"checkpoint tables {tuple(E.shape)}, {tuple(R.shape)} do not fit this model")
    if not reset_optimizer:
        want, have = ("adam" if _is_adam(step) else "adagrad"), _checkpoint_optimizer(ckpt)
        if want != have:
            raise ValueError(f"the checkpoint holds {have} optimizer state and this step trains with {want}: its accumulators do "
                             f"not carry over -- load with reset_optimizer=True to take the tables alone")
    if hasattr(step, "flush"):                                    # deferred weight decay: no row may owe steps to the loaded tables
        step.flush()
    step.E.copy_(E[lo:hi])
    step.R.copy_(R)
    if _is_adam(step):
        _load_adam_state(step, None if reset_optimizer else ckpt["optimizer_state_dict"][0]["optimizer_state"], ckpt)
    elif reset_optimizer:
        step.sumE.zero_()
        step.sumR.zero_()
        step.steps = 0
    else:
        st = ckpt["optimizer_state_dict"][0]["optimizer_state"]
        group, state = st["param_groups"][0], st["state"]
        step.sumE.copy_(state[0]["sum"][lo:hi])
        step.sumR.copy_(state[1]["sum"])
        step.steps = int(float(state[0]["step"]))
        step.lr, step.weight_decay, step.eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
        if float(group.get("lr_decay", 0)) != 0 or float(group.get("initial_accumulator_value", 0)) != 0:
            raise NotImplementedError("Adagrad lr_decay / initial_accumulator_value are not used by the reference configs")
    if step.dE is not None:                                       # (the row-sparse step keeps no dense gradients)
        step.dE.zero_()
        step.dR.zero_()
    return ckpt


def _load_adam_state(step, st, ckpt):
    """moments, t and hyper-parameters of an Adam step from torch.optim.Adam's state (None: reset -- zero moments, t = 0)"""
    if st is None or 0 not in st["state"]:                       # (a torch optimizer that has not stepped yet holds no state)
        for x in (step.mE, step.vE, step.mR, step.vR):
            x.zero_()
        step.set_adam_t(0)
        step.steps = 0
        return
    group, state = st["param_groups"][0], st["state"]
    if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
        raise NotImplementedError("amsgrad, maximize and decoupled weight decay (AdamW) are not implemented")
    step.mE.copy_(state[0]["exp_avg"])
    step.vE.copy_(state[0]["exp_avg_sq"])
    step.mR.copy_(state[1]["exp_avg"])
    step.vR.copy_(state[1]["exp_avg_sq"])
    step.set_adam_t(int(float(state[0]["step"])))
    step.steps = int(ckpt.get("training_steps", int(float(state[0]["step"]))))
    step.lr, step.weight_decay, step.eps = float(group["lr"]), float(group["weight_decay"]), float(group["eps"])
    step.betas = (float(group["betas"][0]), float(group["betas"][1]))
