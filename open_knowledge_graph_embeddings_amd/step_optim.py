"""The optimizer side of the steps that train more than two tensors (virtual_tables.VirtualTableStep and its subclasses,
tucker3.Tucker3TrainStep): the keywords `optimizer`, `betas` and `grad_clip` of train_step.FusedTrainStep, through the
multi-tensor calls okge_adam_multi and okge_clip_grad_norm_multi.

A step says which tensors its optimizer moves -- `_param_groups(every=False)` -> [(p, g, state_sum[, touched_map, stamp]), ...],
the list its Adagrad launch takes; every=True: also those of a slot the scorer leaves unused -- and calls `_update(groups)`
where it called adagrad_multi.  With the defaults (optimizer="adagrad", grad_clip=0) nothing is allocated and `_update` IS that
one call.
"""
from __future__ import annotations

import torch

from . import hotpath as H

ADAGRAD_MAX, ADAM_MAX = 4, 4          # tensors per okge_adagrad_multi / okge_adam_multi launch


def check_optimizer(optimizer, betas):
    """-> (name, betas) as FusedTrainStep spells and refuses them"""
    name = str(optimizer).lower()
    if name not in ("adagrad", "adam"):
        raise ValueError(f"optimizer {optimizer!r}: 'adagrad' or 'adam'")
    b = (float(betas[0]), float(betas[1]))
    if name == "adam" and not (0.0 <= b[0] < 1.0 and 0.0 <= b[1] < 1.0):
        raise ValueError(f"Invalid beta parameters: {betas}")
    return name, b


def refuse_single_device(inner, who):
    """a step that is built for eager single-device use says so in `single_device` (what to use instead): no wrapper takes it"""
    why = getattr(inner, "single_device", None)
    if why:
        raise NotImplementedError(f"{who}: {why}")


def refuse_for_replicas(inner, who):
    """sharded.ReplicaStep: the exchange is built for the Adagrad step without clipping"""
    refuse_single_device(inner, who)
    if isinstance(inner, StepOptimizer) and (inner.optimizer != "adagrad" or inner.grad_clip > 0):
        raise NotImplementedError(f"{who}: optimizer='adam' and grad_clip are built for the single-device steps")
    if getattr(inner, "freeze", None) is not None:
        raise NotImplementedError(f"{who}: an inner step with a frozen table (freeze={inner.freeze!r}) is built for a single device "
                                  f"(the exchange moves both tables' gradients); build the inner step with freeze=None")
    if getattr(inner, "deterministic", False):
        raise NotImplementedError(f"{who}: a deterministic inner step is built for a single device (the exchange adds the replicas' "
                                  f"gradients in an order of its own); build the inner step with deterministic=False")


def state_views(states, offset, param):
    """the part of each flat state tensor that belongs to `param`: `param.numel()` elements from `offset`, in its shape (views)"""
    return tuple(s.reshape(-1)[offset:offset + param.numel()].view(param.shape) for s in states)


class StepOptimizer:
    """mixin: needs self.engine, self.device, self.lr / weight_decay / eps and _param_groups()"""

    optimizer, betas, grad_clip, grad_norm = "adagrad", (0.9, 0.999), 0.0, None

    def _init_optimizer(self, optimizer, betas, grad_clip):
        """after the step's tensors exist.  Adam: per tensor exp_avg, exp_avg_sq (zeros) and a device state (HotPath.adam_state;
        [0] = t, the steps taken, counted on the device so that a captured graph replays it); the Adagrad accumulators are left
        alone.  grad_clip > 0: the norm of the last clipped step stays in self.grad_norm (device double[1])."""
        self.optimizer, self.betas = check_optimizer(optimizer, betas)
        self.grad_clip = float(grad_clip or 0.0)
        if self.grad_clip > 0:
            self.grad_norm = torch.zeros(1, dtype=torch.float64, device=self.device)
        if self.optimizer == "adam":
            self._adam = {t[0].data_ptr(): (torch.zeros_like(t[0]), torch.zeros_like(t[0]), H.HotPath.adam_state(self.device))
                          for t in self._param_groups(every=True)}

    def adam_tensors(self, every=False):
        """[(p, g, exp_avg, exp_avg_sq, state), ...] in the order of _param_groups"""
        return [(t[0], t[1]) + self._adam[t[0].data_ptr()] for t in self._param_groups(every=every)]

    def _optimizer_state(self):
        """what state_tensors() lists on top of parameters, gradients and accumulators: moments and device states"""
        if self.optimizer != "adam":
            return []
        return [x for m, v, st in self._adam.values() for x in (m, v, st)]

    @property
    def adam_t(self):
        """optimizer steps the Adam state has taken (read back from the device: synchronises)"""
        return int(next(iter(self._adam.values()))[2][0].item())

    def set_adam_t(self, t):
        """every tensor's device step count (a loaded checkpoint, a reset)"""
        for _, _, st in self._adam.values():
            st.zero_()
            st[0] = int(t)

    # -- what checkpoint.py needs (through the embedders' optimizer_params_and_state) -----------------------------------
    def optimizer_state_of(self, p, state_sum):
        """the optimizer's state tensors of one entry (p, g, state_sum, ...) of _param_groups(): (state_sum,) under Adagrad,
        (exp_avg, exp_avg_sq) under Adam -- each of p's shape"""
        if self.optimizer == "adam":
            return self._adam[p.data_ptr()][:2]
        return (state_sum,)

    def adam_word(self):
        """the device state word the Adam kernels count their steps in ([0] = t; every tensor's holds the same count), or None"""
        return next(iter(self._adam.values()))[2] if self.optimizer == "adam" else None

    def reset_gradients(self):
        """gradient buffers and touched-row maps as the head of a step expects them: all zero"""
        for t in self._param_groups(every=True):
            t[1].zero_()
            if len(t) > 3 and t[3] is not None:
                t[3].zero_()

    def sync_module(self):
        """before an attached module's state_dict is read: deferred updates settled; a step that keeps copies of module state
        (virtual_tables.VirtualTableStep) brings the module up to date"""
        self.flush()

    def adopt_module(self):
        """after an attached module's state_dict was loaded: such copies follow the module (none here)"""

    def _clip(self, groups):
        """trainer.py:236-240: clip_grad_norm_ over exactly the gradients the update that follows reads, maps included"""
        if self.grad_clip > 0:
            self.engine.clip_grad_norm_multi_([(t[1], t[3], t[4]) if len(t) > 3 and t[3] is not None else t[1] for t in groups],
                                              self.grad_clip, self.grad_norm)

    def _update(self, groups):
        """clip (grad_clip > 0), then Adagrad or Adam over `groups`, at most four tensors per launch"""
        self._clip(groups)
        if self.optimizer == "adam":
            tensors = [(t[0], t[1]) + self._adam[t[0].data_ptr()] + tuple(t[3:5]) for t in groups]
            for i in range(0, len(tensors), ADAM_MAX):
                self.engine.adam_multi(tensors[i:i + ADAM_MAX], self.lr, self.betas, self.eps, self.weight_decay)
            return
        for i in range(0, len(groups), ADAGRAD_MAX):
            self.engine.adagrad_multi(groups[i:i + ADAGRAD_MAX], self.lr, self.weight_decay, self.eps)
