"""HIP encode and training step for the lookup embedder's `_encode` variants (openkge/model.py:455-480): batch_norm,
project_entity, normalize='norm' and the l2_reg hook of Lookup{Complex,Distmult}RelationModel, over the kernels of
csrc/okge_lookup_encode.hip.

One pass encodes the five calls of a batch (trainer.py:75-91: candidates, po relations, po objects, sp subjects, sp relations)
straight into the virtual tables of virtual_tables.py; the fused step runs on them with the FINAL dropout's five masks
(model.py:469-470), okge_n3_forward_backward adds the hook (model.py:471-479) on the same rows, and the pass's backward carries
dEV / dRV through normalisation, projection, batch-norm and the input-dropout mask into the dense table gradients.  The input
dropout (model.py:461-462) draws from five Philox streams of its own (INPUT_STREAMS).

Not built here (refused with a message): project_relation (Tucker3: tucker3.py), sparse=True, slot sizes above 512 (the fused
tile kernels' limit), entity_embedding_size != entity_slot_size, activations other than ReLU / None, per-direction candidate
blocks (batch_shared_entities=None in training: AddLossModule keeps the torch fall-through for those batches), GraphedTrainStep /
ReplicaStep / the sharded steps around this step.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N
from . import hotpath as H
from . import virtual_tables as VT
from .step_optim import state_views

MAX_SLOT = 512                                      # the fused tile kernels' largest slot size (token_encoder.MAX_SLOT)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1                     # torch.nn.BatchNorm1d's defaults (model.py:437-439)
# input-dropout streams of the five encode calls, in the order of virtual_tables.encode_calls (include/okge.h,
# OKGE_LOOKUP_STREAM_*): candidates, po relations, po objects, sp subjects, sp relations
INPUT_STREAMS = (16, 18, 17, 19, 20)
_SUBJ_CALL = 3                                      # the call that takes subj_projection


def refuse_unsupported(model):
    """what the HIP encode does not cover, each with what to use instead"""
    if getattr(model, "project_relation", False):
        raise NotImplementedError("project_relation (the Tucker3 model) is not part of the lookup variants' HIP encode: "
                                  "LookupTucker3RelationModel.train_step() returns its own Tucker3TrainStep")
    if model.entity_embedding.weight.is_sparse or getattr(model.entity_embedding, "sparse", False):
        raise NotImplementedError("sparse=True is not built for the lookup variants: use the row-sparse step of a plain lookup model")
    d = model.slot_size
    if d > MAX_SLOT:
        raise NotImplementedError(f"slot sizes above {MAX_SLOT} are not built for the lookup variants' HIP encode (the virtual-table "
                                  f"fused call stops there): train through AddLossModule's torch fall-through")
    if model.entity_embedding.weight.shape[1] != d:
        raise NotImplementedError("entity_embedding_size != entity_slot_size is not built for the lookup variants' HIP encode: "
                                  "train through AddLossModule's torch fall-through")


def activation_name(model):
    """'ReLU' / None of the model's entity projection; anything else is refused"""
    if not model.project_entity:
        return None
    layers = list(model.obj_projection)[1:]
    if not layers:
        return None
    if len(layers) == 1 and isinstance(layers[0], torch.nn.ReLU):
        return "ReLU"
    raise NotImplementedError(f"project_entity_activation {type(layers[0]).__name__!r}: the HIP encode builds 'ReLU' and None; "
                              f"train through AddLossModule's torch fall-through")


class LookupSlot:
    """One embedder slot: the table, its gradient and accumulator, and the slot's BatchNorm1d -- (weight, bias) in `bn`, their
    gradients and accumulators, the running statistics -- or bn = None.  All parameters are the module's own storage."""

    bn_calls = 0      # training-mode batch-norm encode calls since VirtualTableStep.sync_module (host count)

    def __init__(self, W, bn=None, running=None):
        self.W, self.d = W, W.shape[1]
        self.bn = None if bn is None else (bn[0], bn[1])
        if bn is not None:
            self.running_mean, self.running_var = running
        self.fresh_grads()
        self.sumW = torch.zeros_like(W)
        self.sum_bn = None if bn is None else (torch.zeros_like(bn[0]), torch.zeros_like(bn[1]))

    def fresh_grads(self):
        self.dW = torch.zeros_like(self.W)
        self.d_bn = None if self.bn is None else (torch.zeros_like(self.bn[0]), torch.zeros_like(self.bn[1]))

    def optimizer_tensors(self):
        out = [(self.W, self.dW, self.sumW)]
        if self.bn is not None:
            out += [(p, g, s) for p, g, s in zip(self.bn, self.d_bn, self.sum_bn)]
        return out


class LookupVariantTrainStep(VT.VirtualTableStep):
    """forward + loss + backward + Adagrad / Adam for a Lookup{Complex,Distmult}RelationModel with batch_norm, project_entity,
    normalize='norm' or l2_reg on (Trainer.compute_one_batch, trainer.py:181-257, over model.py:455-480).

    entity / relation: LookupSlot; projection: (W_subj, W_obj) -- the (d, d) weights of subj_projection / obj_projection -- or None;
    activation: 'ReLU' or None behind the projection; normalize: '' or 'norm'; l2_reg: the hook's factor (its value of the last
    step stays in self.reg_out, a device double[1]); input_dropout / relation_input_dropout: the dropout in FRONT of the
    batch-norm; dropout / relation_dropout: the final one.  optimizer / betas / grad_clip as on FusedTrainStep: every tensor of
    _param_groups() moves every step."""

    single_device = ("LookupVariantTrainStep is built for eager steps on one device (its backward sorts the batch's ids on the way and "
                     "its batch-norm call counts live on the host): call step() directly, or train a plain lookup model through "
                     "FusedTrainStep / ReplicaTrainStep")

    def __init__(self, entity, relation, scorer, projection=None, activation="ReLU", normalize="", l2_reg=0.0, input_dropout=0.0,
                 relation_input_dropout=None, **kwargs):
        if scorer not in ("complex", "distmult"):
            raise NotImplementedError(f"LookupVariantTrainStep is built for the ComplEx and DistMult scorers, not {scorer!r}")
        if activation not in (None, "ReLU"):
            raise NotImplementedError(f"project_entity_activation {activation!r}: the HIP encode builds 'ReLU' and None")
        if normalize not in ("", None, "norm"):
            raise NotImplementedError(f"normalize={normalize!r}")
        if entity.d > MAX_SLOT:
            raise NotImplementedError(f"slot sizes above {MAX_SLOT} are not built for the lookup variants' HIP encode")
        if entity.d != relation.d or (entity.bn is None) != (relation.bn is None):
            raise ValueError("the two slots share the slot size and the batch_norm switch")
        self.projection = None
        if projection is not None:
            self.projection = tuple(projection)                      # (W_subj, W_obj)
            if any(tuple(w.shape) != (entity.d, entity.d) for w in self.projection):
                raise NotImplementedError("entity_embedding_size != entity_slot_size is not built for the HIP encode")
            self.sum_proj = tuple(torch.zeros_like(w) for w in self.projection)
            self.fresh_projection_grads()
        self.activation, self.normalize, self.l2_reg = activation, normalize or "", float(l2_reg or 0.0)
        self.input_dropout = float(input_dropout)
        self.relation_input_dropout = self.input_dropout if relation_input_dropout is None else float(relation_input_dropout)
        self.lib = N.lib()
        self.ws, self.ws_bytes = None, 0
        self._list_rows = {}
        super().__init__(entity, relation, scorer, **kwargs)
        self.reg_out = torch.zeros(1, dtype=torch.float64, device=self.device)
        self._normalizer = None

    def fresh_projection_grads(self):
        self.d_proj = tuple(torch.zeros_like(w) for w in self.projection)

    # -- optimizer ---------------------------------------------------------------------------------------------------------
    def _param_groups(self, every=False):
        """E, R, the batch-norm parameters of both slots, both projection weights"""
        out = self.entity.optimizer_tensors()[:1] + self.relation.optimizer_tensors()[:1]
        out += self.entity.optimizer_tensors()[1:] + self.relation.optimizer_tensors()[1:]
        if self.projection is not None:
            out += list(zip(self.projection, self.d_proj, self.sum_proj))
        return out

    def state_tensors(self):
        out = [x for t in self._param_groups(every=True) for x in t]
        for sl in (self.entity, self.relation):
            if sl.bn is not None:
                out += [sl.running_mean, sl.running_var]
        return out + self._optimizer_state()

    def flush(self):
        """(no deferred updates here: every parameter is current after every step)"""

    def optimizer_step(self):
        self._update(self._param_groups())

    def _sync_module_batchnorms(self):
        """(the slots' batch-norm parameters and running statistics ARE the attached module's tensors)"""

    def adopt_module(self):
        for sl, _ in self.module_batchnorms:
            sl.bn_calls = 0

    # -- the pass ----------------------------------------------------------------------------------------------------------
    def _encoder(self):
        e = N.LookupEncoder()
        E, R = self.entity.W, self.relation.W
        e.E, e.R, e.n_ent, e.n_rel, e.d = E.data_ptr(), R.data_ptr(), E.shape[0], R.shape[0], self.entity.d
        e.normalize, e.activation = int(self.normalize == "norm"), int(self.activation == "ReLU")
        if self.entity.bn is not None:
            for tag, sl in (("e", self.entity), ("r", self.relation)):
                setattr(e, f"bn_{tag}_weight", sl.bn[0].data_ptr())
                setattr(e, f"bn_{tag}_bias", sl.bn[1].data_ptr())
                setattr(e, f"bn_{tag}_running_mean", sl.running_mean.data_ptr())
                setattr(e, f"bn_{tag}_running_var", sl.running_var.data_ptr())
        if self.projection is not None:
            e.W_subj, e.W_obj = self.projection[0].data_ptr(), self.projection[1].data_ptr()
        e.bn_eps, e.bn_momentum = BN_EPS, BN_MOMENTUM
        return e

    def _calls(self, batch, training):
        """-> (the five okge_lookup_call, the id tensors they point into, entity rows, relation rows)"""
        arr, keep, rows = (N.LookupCall * 5)(), [], [0, 0]
        for i, (c, (relation, ids, first, span)) in enumerate(zip(arr, VT.encode_calls(batch))):
            n = span.stop - span.start
            ids = H._i32(ids, self.device) if n else None
            keep.append(ids)
            c.ids, c.first_id, c.n = (None if ids is None else ids.data_ptr()), int(first), n
            c.relation, c.subj = int(relation), int(i == _SUBJ_CALL)
            p = (self.relation_input_dropout if relation else self.input_dropout) if training else 0.0
            H.DropoutSpec(p, self.seed, INPUT_STREAMS[i], self.steps, step_dev=self.step_dev).fill(c.input_drop)
            rows[relation] += n
            if training and n == 1 and self.entity.bn is not None:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size torch.Size([1, {self.entity.d}])")
        return arr, keep, rows[0], rows[1]

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _rows(self, bufs):
        """the buffers the skeleton hands to the fused call: EV / RV behind a batch-norm, EX / RX otherwise"""
        EV, EX, dEV, RV, RX, dRV = bufs
        return (EV if self.entity.bn is not None else EX), (RV if self.relation.bn is not None else RX)

    def _encode(self, batch, bufs, training=True):
        arr, keep, n_e, n_r = self._calls(batch, training)           # (raises before any launch)
        need = int(self.lib.okge_lookup_workspace_bytes(n_e, n_r, self.entity.d, int(training)))
        if need == 0:
            raise N.OkgeError(f"invalid lookup pass: {n_e} entity rows, {n_r} relation rows, d = {self.entity.d}")
        if need > self.ws_bytes:
            self.ws, self.ws_bytes = torch.empty(need, dtype=torch.uint8, device=self.device), need
        V_e, V_r = self._rows(bufs)
        enc = self._encoder()
        N.check(self.lib.okge_lookup_encode_calls(ctypes.byref(enc), arr, 5, int(training), V_e.data_ptr(), V_e.stride(0), V_r.data_ptr(),
                                                  V_r.stride(0), self.ws.data_ptr(), self.ws_bytes, self._stream()),
                "okge_lookup_encode_calls")
        if training and self.entity.bn is not None:
            for c in arr:
                if c.n:
                    (self.relation if c.relation else self.entity).bn_calls += 1
        return enc, arr, keep

    def _list_order(self, batch, keep):
        """the pass's id-list rows (numbered entity calls first, then relation calls) sorted by (table, id), stable: index
        plumbing on the device, the sums are the kernel's"""
        n_c, n_po, n_sp = batch.n_candidates, batch.n_po, batch.n_sp
        key = (n_c, n_po, n_sp, batch.cand_ids is None)
        if key not in self._list_rows:
            spans = VT.row_ranges(n_c, n_po, n_sp)
            n_e = n_c + n_po + n_sp
            parts, shift = [], []
            for i, (ids, span) in enumerate(zip(keep, spans)):
                if ids is None:
                    continue
                relation = i in (1, 4)
                parts.append(torch.arange(span.start, span.stop, dtype=torch.int64, device=self.device) + (n_e if relation else 0))
                shift.append(torch.full((span.stop - span.start,), int(relation) << 32, dtype=torch.int64, device=self.device))
            self._list_rows = {key: (torch.cat(parts), torch.cat(shift)) if parts else None}
        rows = self._list_rows[key]
        if rows is None:
            return None, 0
        ids = torch.cat([x for x in keep if x is not None]).to(torch.int64) & 0xFFFFFFFF
        order = rows[0][torch.argsort(ids + rows[1], stable=True)].to(torch.int32)
        return order, int(order.numel())

    def forward_backward(self, batch, normalizer=None, scores=None):
        self._normalizer = normalizer
        return super().forward_backward(batch, normalizer, scores)

    def _backward(self, batch, bufs, saved):
        """the l2_reg hook on the rows the fused call just read (same masks), then dEV / dRV -> the slots' gradients"""
        enc, arr, keep = saved
        EV, EX, dEV, RV, RX, dRV = bufs
        V_e, V_r = self._rows(bufs)
        if self.l2_reg > 0:
            vb = self.tables.batch(batch.n_candidates, batch.n_po, batch.n_sp, batch.pos_row, batch.pos_col,
                                   H.dropout_specs(self.dropout, self.relation_dropout, self.seed, self.steps, self.step_dev))
            self.engine.n3_forward_backward(V_e, V_r, self.scorer, vb, dEV, dRV, H.n3_coef(self.l2_reg, self.dropout), cand_passes=1,
                                            normalizer=self._normalizer, reg_out=self.reg_out, distinct_prefix_rows=True)
        order, n_list = self._list_order(batch, keep)
        ptr = lambda t: None if t is None else t.data_ptr()            # noqa: E731
        e_bn, r_bn = self.entity.d_bn or (None, None), self.relation.d_bn or (None, None)
        d_subj, d_obj = self.d_proj if self.projection is not None else (None, None)
        N.check(self.lib.okge_lookup_backward_calls(
            ctypes.byref(enc), arr, 5, V_e.data_ptr(), V_e.stride(0), V_r.data_ptr(), V_r.stride(0), dEV.data_ptr(), dEV.stride(0),
            dRV.data_ptr(), dRV.stride(0), ptr(order), n_list, self.entity.dW.data_ptr(), self.relation.dW.data_ptr(), ptr(e_bn[0]),
            ptr(e_bn[1]), ptr(r_bn[0]), ptr(r_bn[1]), ptr(d_obj), ptr(d_subj), self.ws.data_ptr(), self.ws_bytes, self._stream()),
            "okge_lookup_backward_calls")

    def loss_only(self, batch, scores=None, normalizer=1.0):
        """eval-mode forward + summed loss (running statistics, no dropout, no hook): the validation loss (trainer.py:363-369)"""
        shape = (batch.n_candidates, batch.n_po, batch.n_sp)
        bufs = self.tables.buffers(*shape, self.entity.d)
        self._encode(batch, bufs, training=False)
        V_e, V_r = self._rows(bufs)
        vb = self.tables.batch(*shape, batch.pos_row, batch.pos_col)
        return self.engine.forward_backward(V_e, V_r, self.scorer, vb, None, None, loss=self.loss, label_smoothing=self.label_smoothing,
                                            normalizer=normalizer, loss_out=self.loss_out, scores=scores, loss_only=True)


# ----------------------------------------------------------------------------------------------------------------------
# the lookup models' side (model.LookupBaseRelationEmbedder calls these)
# ----------------------------------------------------------------------------------------------------------------------
def _slots(model):
    bn_e, bn_r = (model.bn_e, model.bn_r) if model.batch_norm else (None, None)
    mk = lambda emb, bn: LookupSlot(emb.weight.data, None if bn is None else (bn.weight.data, bn.bias.data),      # noqa: E731
                                    None if bn is None else (bn.running_mean, bn.running_var))
    return mk(model.entity_embedding, bn_e), mk(model.relation_embedding, bn_r)


def make_step(model, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8, label_smoothing=0.0, optimizer="adagrad", betas=(0.9, 0.999),
              grad_clip=0.0):
    """LookupVariantTrainStep bound to the module's parameters (updated in place)"""
    if not model.encode_in_torch:
        raise ValueError("this lookup model has no _encode variant on (batch_norm, project_entity, normalize, l2_reg): its training "
                         "driver is train_step.FusedTrainStep")
    refuse_unsupported(model)
    activation = activation_name(model)
    entity, relation = _slots(model)
    projection = None
    if model.project_entity:
        projection = (model.subj_projection[0].weight.data, model.obj_projection[0].weight.data)
    st = LookupVariantTrainStep(entity, relation, model.scorer_name, projection=projection, activation=activation,
                                normalize=model.normalize, l2_reg=model.l2_reg, input_dropout=model.input_dropout,
                                relation_input_dropout=model.relation_input_dropout, loss=loss, lr=lr, weight_decay=weight_decay, eps=eps,
                                label_smoothing=label_smoothing, dropout=model.dropout, relation_dropout=model.relation_dropout,
                                seed=model.dropout_seed, engine=model.engine(), optimizer=optimizer, betas=betas, grad_clip=grad_clip)
    if model.batch_norm:
        st.module_batchnorms = ((entity, model.bn_e), (relation, model.bn_r))
    return st


def _step_parameters(model, st):
    """[(module parameter, the step's (p, g, state_sum) entry of it)]"""
    groups = st._param_groups(every=True)
    params = [model.entity_embedding.weight, model.relation_embedding.weight]
    if model.batch_norm:
        params += [model.bn_e.weight, model.bn_e.bias, model.bn_r.weight, model.bn_r.bias]
    if model.project_entity:
        params += [model.subj_projection[0].weight, model.obj_projection[0].weight]
    return list(zip(params, groups))


def autograd_step(model, loss, label_smoothing):
    """the cached step behind AddLossModule(fused_variants=True): shares the module's parameters; its optimizer is NOT used (the
    caller's torch optimizer steps the module parameters); fresh gradient buffers every call (the last ones went to autograd)"""
    st = getattr(model, "_ag_step", None)
    if st is None or st.loss != loss or st.label_smoothing != label_smoothing or \
            any(p.data_ptr() != g[0].data_ptr() for p, g in _step_parameters(model, st)) or \
            (model.batch_norm and st.entity.running_mean.data_ptr() != model.bn_e.running_mean.data_ptr()):
        st = model._ag_step = make_step(model, loss=loss, label_smoothing=label_smoothing)
    else:
        st.entity.fresh_grads()
        st.relation.fresh_grads()
        if st.projection is not None:
            st.fresh_projection_grads()
    st.l2_reg = float(model.l2_reg or 0.0)
    st.dropout, st.relation_dropout = model.dropout, model.relation_dropout
    st.input_dropout, st.relation_input_dropout = model.input_dropout, model.relation_input_dropout
    st.steps = model.dropout_step
    model.dropout_step += 1
    return st


def autograd_params_and_grads(model, st):
    pairs = _step_parameters(model, st)
    return [p for p, _ in pairs], [g[1] for _, g in pairs]


def loss_only(model, batch, kind, smoothing, all_outputs):
    step = model.dropout_step
    st = autograd_step(model, kind, smoothing)                      # (the cached step; no mask is drawn here)
    model.dropout_step = step
    return st.loss_only(batch, scores=all_outputs, normalizer=1.0)


def optimizer_params_and_state(model, st):
    """For checkpoint.py (see tucker3.ProjectedLookupRelationEmbedder.optimizer_params_and_state)"""
    if not isinstance(st, LookupVariantTrainStep):
        raise TypeError(f"model_checkpoint / load_model_checkpoint take a lookup model with an _encode variant on and the driver its "
                        f"train_step() returned, not {type(st).__name__}: the two-table lookup steps go through "
                        f"to_reference_checkpoint / load_reference_checkpoint")
    found = {p: state_views(st.optimizer_state_of(g[0], g[2]), 0, p) for p, g in _step_parameters(model, st)}
    return [(p, tuple(found[p]), True) for p in model.parameters()], st.adam_word()
