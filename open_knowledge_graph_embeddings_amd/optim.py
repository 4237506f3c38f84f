"""`OkgeAdagrad`: torch.optim.Adagrad's dense update (the optimizer OptimRegime builds for every reference config,
utils/optim.py:139-160) on the HIP sweep kernel -- one launch per PAIR of parameters instead of ATen's foreach chain -- and
its sparse branch (row-sparse gradients at weight_decay = 0) on okge_adagrad_rows.

The reference names its optimizer in YAML (`optimization_config.optimizer`) and looks the class up in
`torch.optim.__dict__` (utils/optim.py:143-144), constructing it from the PREVIOUS optimizer's param_groups -- which is
how Adam's eps = 1e-8 leaks into Adagrad.  Importing this module registers the class there, so
`optimizer: OkgeAdagrad` in a config selects it and the leaked keys are honoured the same way (torch's Optimizer keeps
keys a group already has).  State layout = torch.optim.Adagrad's ({'step', 'sum'} per parameter), so checkpoints move
between the two.

`OkgeAdam` / `OkgeSparseAdam`: the same for `optimizer: Adam` -- torch.optim.Adam's dense update (coupled weight decay, no
amsgrad) on okge_adam_step and torch.optim.SparseAdam's on okge_adam_rows, registered the same way, state layout
{'step', 'exp_avg', 'exp_avg_sq'}."""
from __future__ import annotations

import torch

from . import hotpath as H


class OkgeAdagrad(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-2, lr_decay=0, weight_decay=0, initial_accumulator_value=0, eps=1e-10):
        defaults = dict(lr=lr, lr_decay=lr_decay, eps=eps, weight_decay=weight_decay,
                        initial_accumulator_value=initial_accumulator_value)
        super().__init__(params, defaults)
        self._engines = {}
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state[p]
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["sum"] = torch.full_like(p, float(group["initial_accumulator_value"]), memory_format=torch.preserve_format)

    def _engine(self, dev):
        if dev not in self._engines:
            self._engines[dev] = H.HotPath(dev)
        return self._engines[dev]

    def zero_grad(self, set_to_none: bool = True):
        """torch.optim.Optimizer.zero_grad(set_to_none=True) without its profiler scope and foreach bookkeeping (~15 us of
        host time per step on a 130 us device step); anything else goes to the base class"""
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for group in self.param_groups:
            for p in group["params"]:
                p.grad = None

    def step(self, closure=None):
        """One Adagrad update.  torch wraps every optimizer's `step` in a profiler scope + hook dispatch
        (Optimizer.profile_hook_step, ~30 us of host time per call); this class opts out of the wrapper (`hooked` below)
        and pays for it only when step hooks are actually registered."""
        if self._optimizer_step_pre_hooks or self._optimizer_step_post_hooks or _global_step_hooks():
            return torch.optim.Optimizer.profile_hook_step(OkgeAdagrad._step)(self, closure)
        return self._step(closure)

    @torch.no_grad()
    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            todo, rows = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if g.is_sparse and group["weight_decay"] != 0:      # (torch.optim.Adagrad's own refusal and text)
                    raise RuntimeError("weight_decay option is not compatible with sparse gradients")
                if p.dtype != torch.float32 or g.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                    raise RuntimeError("OkgeAdagrad updates dense contiguous fp32 parameters on the GPU")
                if g.is_sparse and (p.dim() != 2 or g.sparse_dim() != 1):
                    raise RuntimeError("OkgeAdagrad takes row-sparse gradients (one sparse dimension) of 2-d parameters")
                st = self.state[p]
                if st["sum"].device != p.device:
                    st["sum"] = st["sum"].to(p.device)
                st["step"] += 1
                if g.is_sparse:                # (uncoalesced, as nn.Embedding(sparse=True) / AddLossModule(sparse_grads=True) leave it)
                    rows.append((p, g, st))
                else:
                    todo.append((p, g if g.is_contiguous() else g.contiguous(), st))
            self._step_rows(group, rows)
            if not todo:
                continue
            if group["lr_decay"] != 0:
                clrs = [group["lr"] / (1 + (float(st["step"]) - 1) * group["lr_decay"]) for _, _, st in todo]
            else:
                clrs = [group["lr"]] * len(todo)
            eng = self._engine(todo[0][0].device)
            i = 0
            while i < len(todo):
                if i + 1 < len(todo) and clrs[i] == clrs[i + 1]:
                    (p0, g0, s0), (p1, g1, s1) = todo[i], todo[i + 1]
                    eng.adagrad2(p0.data, g0, s0["sum"], p1.data, g1, s1["sum"], clrs[i], group["weight_decay"], group["eps"],
                                 zero_grad=False)
                    i += 2
                else:
                    p0, g0, s0 = todo[i]
                    eng.adagrad(p0.data, g0, s0["sum"], clrs[i], group["weight_decay"], group["eps"], zero_grad=False)
                    i += 1
        return loss

    def _step_rows(self, group, rows):
        """torch.optim.Adagrad's sparse branch on okge_adagrad_rows: the value rows are coalesced per index in ascending
        position and only the rows they name are updated; `sum` stays dense (the state layout does not change).  Two
        parameters of one learning rate share the launches."""
        i = 0
        while i < len(rows):
            p0, g0, s0 = rows[i]
            clr = group["lr"] / (1 + (float(s0["step"]) - 1) * group["lr_decay"]) if group["lr_decay"] != 0 else group["lr"]
            second = None
            if i + 1 < len(rows):
                p1, g1, s1 = rows[i + 1]
                clr1 = group["lr"] / (1 + (float(s1["step"]) - 1) * group["lr_decay"]) if group["lr_decay"] != 0 else group["lr"]
                if clr1 == clr:
                    second = (p1.data, s1["sum"], _row_ids(g1), _row_values(g1))
            self._engine(p0.device).adagrad_rows(p0.data, s0["sum"], _row_ids(g0), _row_values(g0), clr, group["eps"], second=second)
            i += 2 if second is not None else 1


def _row_ids(g):
    return g._indices()[0].to(torch.int32).contiguous()


def _row_values(g):
    v = g._values()
    return v if v.dim() == 2 and v.stride(1) == 1 else v.reshape(v.shape[0], -1).contiguous()


import sys as _sys

_optim_mod = _sys.modules[torch.optim.Optimizer.__module__]       # torch.optim.optimizer (the submodule, not the re-export)


def _global_step_hooks():
    return bool(getattr(_optim_mod, "_global_optimizer_pre_hooks", None)) or \
        bool(getattr(_optim_mod, "_global_optimizer_post_hooks", None))


OkgeAdagrad.step.hooked = True          # Optimizer._patch_step_function leaves a step marked like this alone


DEVICE_STATE = "okge_state"             # per-parameter key of the device step count; never part of state_dict()


class _OkgeAdamBase(torch.optim.Optimizer):
    """What OkgeAdam and OkgeSparseAdam share: torch's state layout {'step', 'exp_avg', 'exp_avg_sq'} (created on a parameter's
    first step, as torch does) plus the tiny device state the kernels count their steps in -- an extra per-parameter key that
    state_dict() leaves out and that is rebuilt from 'step' after load_state_dict(), so checkpoints move between these classes and
    torch.optim.Adam / SparseAdam.  Group keys the previous optimizer of an OptimRegime leaked (utils/optim.py:145: lr_decay,
    initial_accumulator_value ...) stay in the group unread, as in OkgeAdagrad."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._engines = {}
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError(f"{type(self).__name__}: amsgrad and maximize are not implemented")
            b1, b2 = group["betas"]
            if not (0.0 <= group["lr"] and 0.0 <= group["eps"] and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise ValueError(f"Invalid Adam hyper-parameters: lr {group['lr']}, eps {group['eps']}, betas {group['betas']}")

    _engine = OkgeAdagrad._engine
    zero_grad = OkgeAdagrad.zero_grad

    def step(self, closure=None):
        """(OkgeAdagrad.step's opt-out from torch's hooked wrapper: the profiler scope and hook dispatch are paid only when step
        hooks are registered)"""
        if self._optimizer_step_pre_hooks or self._optimizer_step_post_hooks or _global_step_hooks():
            return torch.optim.Optimizer.profile_hook_step(type(self)._step)(self, closure)
        return self._step(closure)

    def _state(self, p):
        st = self.state[p]
        if "step" not in st:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        for k in ("exp_avg", "exp_avg_sq"):
            if st[k].device != p.device or not st[k].is_contiguous():
                st[k] = st[k].to(p.device).contiguous()
        if DEVICE_STATE not in st or st[DEVICE_STATE].device != p.device:
            st[DEVICE_STATE] = H.HotPath.adam_state(p.device, int(float(st["step"])))
        return st

    def state_dict(self):
        sd = super().state_dict()
        sd["state"] = {k: {kk: vv for kk, vv in v.items() if kk != DEVICE_STATE} for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():              # the device count follows the loaded 'step' (rebuilt at the next step)
            st.pop(DEVICE_STATE, None)
            if "step" in st and torch.is_tensor(st["step"]):
                st["step"] = st["step"].detach().to("cpu", torch.float32).clone()     # (never the tensor of the optimizer it came from)

    def _params(self, group, sparse):
        out = []
        for p in group["params"]:
            if p.grad is None:
                continue
            g = p.grad
            if g.is_sparse != sparse:
                raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead" if g.is_sparse else
                                   "SparseAdam does not support dense gradients, please consider Adam instead")
            if p.dtype != torch.float32 or g.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                raise RuntimeError(f"{type(self).__name__} updates dense contiguous fp32 parameters on the GPU")
            if sparse and (p.dim() != 2 or g.sparse_dim() != 1):
                raise RuntimeError(f"{type(self).__name__} takes row-sparse gradients (one sparse dimension) of 2-d parameters")
            st = self._state(p)
            st["step"] += 1
            out.append((p, g, st))
        return out


class OkgeAdam(_OkgeAdamBase):
    """torch.optim.Adam's dense update (amsgrad = False, maximize = False, coupled weight decay) on okge_adam_step: one launch per
    PAIR of parameters of a group (they share its hyper-parameters; each keeps its own state) instead of ATen's foreach chain."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise NotImplementedError("OkgeAdam: amsgrad and maximize are not implemented")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False))

    @torch.no_grad()
    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            todo = [(p.data, g if g.is_contiguous() else g.contiguous(), st["exp_avg"], st["exp_avg_sq"], st[DEVICE_STATE])
                    for p, g, st in self._params(group, sparse=False)]
            for i in range(0, len(todo), 2):
                self._engine(todo[i][0].device).adam(todo[i:i + 2], group["lr"], group["betas"], group["eps"], group["weight_decay"],
                                                     zero_grad=False)
        return loss


class OkgeSparseAdam(_OkgeAdamBase):
    """torch.optim.SparseAdam on okge_adam_rows: the row-sparse gradients nn.Embedding(sparse=True) / AddLossModule(sparse_grads=True)
    leave (uncoalesced) are coalesced per index in ascending position and only the rows they name move -- reproducibly, where
    SparseAdam's coalesce() is not.  The moments stay dense (torch's layout).  Two parameters of a group share the launches."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, maximize=False):
        if maximize:
            raise NotImplementedError("OkgeSparseAdam: maximize is not implemented")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, maximize=False))

    @torch.no_grad()
    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if group.get("weight_decay", 0) != 0:       # (a key leaked from a dense optimizer; torch's sparse refusal and text)
                raise RuntimeError("weight_decay option is not compatible with sparse gradients")
            todo = [(p.data, st["exp_avg"], st["exp_avg_sq"], st[DEVICE_STATE], _row_ids(g), _row_values(g))
                    for p, g, st in self._params(group, sparse=True)]
            for i in range(0, len(todo), 2):
                self._engine(todo[i][0].device).adam_rows(todo[i:i + 2], group["lr"], group["betas"], group["eps"])
        return loss


_OkgeAdamBase.step.hooked = True


# nameable from the reference's YAML: `optimizer: OkgeAdagrad` -> torch.optim.__dict__["OkgeAdagrad"] (utils/optim.py:143)
torch.optim.OkgeAdagrad = OkgeAdagrad
torch.optim.OkgeAdam = OkgeAdam
torch.optim.OkgeSparseAdam = OkgeSparseAdam
