"""The "virtual tables" of a batch whose rows are ENCODED (pooled, LSTM-encoded, projected ...) instead of looked up, and
the training-step skeleton on top of them.  This module is the one place that knows the layout:

    EV = [candidates | po objects | sp subjects]   (N + n_po + n_sp rows)        RV = [po relations | sp relations]

The unchanged fused step (score -> loss -> backward, dropout included) runs on EV / RV as if they were embedding tables, with
a PrefixBatch of row POSITIONS in place of ids: candidates are the range 0..N-1, every prefix names its own row.  Every row of
the two tables is then one candidate or one batch row, so the call STORES every gradient row (grads_zero: candidate rows by
the tile kernel; distinct_prefix_rows: prefix rows by the prefix backward) and nothing is cleared per step.  Either direction
may be empty.  Nothing here launches a kernel of its own; it works on any torch device.
"""
from __future__ import annotations

import torch

from . import _native as N
from . import hotpath as H
from .step_optim import StepOptimizer, check_optimizer


def row_ranges(n_cand, n_po, n_sp):
    """Rows of the five encode calls, in the reference's call order (trainer.py:75-91): candidates, po relations, po objects,
    sp subjects, sp relations -- the 1st, 3rd and 4th are rows of EV, the 2nd and 5th rows of RV."""
    B = n_po + n_sp
    return slice(0, n_cand), slice(0, n_po), slice(n_cand, n_cand + n_po), slice(n_cand + n_po, n_cand + B), slice(n_po, B)


def encode_calls(batch: H.PrefixBatch):
    """The five encode calls of a batch in that order: (relation slot?, ids or None, first id, rows of EV / RV)."""
    cand, po_rel, po_obj, sp_subj, sp_rel = row_ranges(batch.n_candidates, batch.n_po, batch.n_sp)
    return ((False, batch.cand_ids, batch.cand_first, cand), (True, batch.po_rel, 0, po_rel), (False, batch.po_obj, 0, po_obj),
            (False, batch.sp_subj, 0, sp_subj), (True, batch.sp_rel, 0, sp_rel))


class VirtualTables:
    """Position batches and the growing row buffers of one user (a step, a module) on one device."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._arange = torch.empty(0, dtype=torch.int32, device=self.device)
        self._key, self._positions, self._bufs = None, None, None

    def batch(self, n_cand, n_po, n_sp, pos_row, pos_col, drops=None):
        """The PrefixBatch of positions over EV / RV; positives pass through.  drops: hotpath.dropout_specs(...), or None when
        the encode already applied the dropout.  The positions depend on the shape only: views of one arange, kept for the next
        call of the same shape (four arange launches per step otherwise: 18 us of a 0.9 ms token-pooled step at configs[4])."""
        key = (n_cand, n_po, n_sp)
        if self._key != key:
            if self._arange.numel() < n_cand + n_po + n_sp:
                self._arange = torch.arange(0, n_cand + n_po + n_sp, dtype=torch.int32, device=self.device)
            rng = self._arange
            self._key, self._positions = key, tuple(rng[rows] if rows.stop > rows.start else None for rows in row_ranges(*key)[1:])
        po_rel, po_obj, sp_subj, sp_rel = self._positions
        cand, po_ent, po_r, sp_ent, sp_r = drops or (H.NO_DROP,) * 5
        return H.PrefixBatch(po_rel=po_rel, po_obj=po_obj, sp_subj=sp_subj, sp_rel=sp_rel, pos_row=pos_row, pos_col=pos_col,
                             cand_first=0, n_cand=n_cand, drop_cand=cand, drop_po_ent=po_ent, drop_po_rel=po_r,
                             drop_sp_ent=sp_ent, drop_sp_rel=sp_r)

    def buffers(self, n_cand, n_po, n_sp, d):
        """EV, EX, dEV, RV, RX, dRV trimmed to the batch's rows: encoded rows (after batch-norm), raw rows (before it), row
        gradients.  Reallocated (zeroed) only when a batch needs more rows than any before it."""
        rows = (n_cand + n_po + n_sp,) * 3 + (n_po + n_sp,) * 3
        if self._bufs is None or any(n > b.shape[0] for n, b in zip(rows, self._bufs)):
            self._bufs = tuple(torch.zeros((n, d), device=self.device) for n in rows)
        return tuple(b[:n] for b, n in zip(self._bufs, rows))


class VirtualTableStep(StepOptimizer):
    """Skeleton of a training step that encodes a batch's rows into virtual tables: count the step, get the buffers, `_encode`,
    the fused call on the virtual tables, `_backward`.  A subclass brings optimizer_step() and the two hooks:
        _encode(batch, bufs) -> saved  fill EX / RX (and EV / RV behind a batch-norm) with the batch's rows
        _backward(batch, bufs, saved)  carry dEV / dRV back through the encoder into the slots' gradients
    entity / relation are its slots (.W, .d, .bn or None).  dropout is the entity streams', relation_dropout (default: the
    same) the relation streams' drop probability.  optimizer / betas / grad_clip: as on FusedTrainStep (step_optim.py) -- "adam"
    is torch.optim.Adam's update (coupled weight decay, no amsgrad) over every tensor the step's Adagrad moves, grad_clip > 0
    clips their gradients' global norm at the head of optimizer_step(); a subclass lists the tensors in _param_groups()."""

    bias_scorers = False              # a subclass that leaves a data-bias scorer's unused slot untouched says True

    def __init__(self, entity, relation, scorer, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8, label_smoothing=0.0,
                 dropout=0.0, relation_dropout=None, seed=0, engine=None, optimizer="adagrad", betas=(0.9, 0.999), grad_clip=0.0):
        if not self.bias_scorers:
            N.refuse_bias_scorer(scorer, type(self).__name__)
        check_optimizer(optimizer, betas)
        self.entity, self.relation, self.scorer, self.loss = entity, relation, scorer, loss
        self.lr, self.weight_decay, self.eps, self.label_smoothing = lr, weight_decay, eps, label_smoothing
        self.dropout = dropout
        self.relation_dropout = dropout if relation_dropout is None else relation_dropout
        self.seed, self.steps = seed, 0
        self.device = entity.W.device
        self.engine = engine or H.HotPath(self.device)
        self.tables = VirtualTables(self.device)
        self.loss_out = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.step_dev = None              # device step counter, attached by GraphedTrainStep
        self.module_batchnorms = ()       # ((slot, nn.BatchNorm1d), ...) of an attached module, set by its train_step()
        self._init_optimizer(optimizer, betas, grad_clip)

    def step(self, batch: H.PrefixBatch, normalizer=None):
        """`batch` carries ENTITY / RELATION ids exactly as for the lookup models."""
        loss = self.forward_backward(batch, normalizer)
        self.optimizer_step()
        return loss

    def forward_backward(self, batch: H.PrefixBatch, normalizer=None, scores=None):
        """Leaves the dense gradients in the slots (what `_backward` writes); returns the summed loss, a device double[1]."""
        self.steps += 1
        shape = (batch.n_candidates, batch.n_po, batch.n_sp)
        bufs = self.tables.buffers(*shape, self.entity.d)
        saved = self._encode(batch, bufs)
        EV, EX, dEV, RV, RX, dRV = bufs
        vb = self.tables.batch(*shape, batch.pos_row, batch.pos_col,
                               H.dropout_specs(self.dropout, self.relation_dropout, self.seed, self.steps, self.step_dev))
        self.engine.forward_backward(EV if self.entity.bn is not None else EX, RV if self.relation.bn is not None else RX,
                                     self.scorer, vb, dEV, dRV, loss=self.loss, label_smoothing=self.label_smoothing,
                                     normalizer=normalizer, loss_out=self.loss_out, scores=scores, grads_zero=True,
                                     distinct_prefix_rows=True)
        self._backward(batch, bufs, saved)
        return self.loss_out

    def _unused(self, sl):
        """whether the scorer leaves this slot out of the score (its parameters then have no gradient and do not move)"""
        return False

    def _sync_module_batchnorms(self):
        """after an optimizer step: keep an attached nn.Module's batch-norm parameters current"""
        for sl, bn in self.module_batchnorms:
            bn.weight.data.copy_(sl.bn[:sl.d])
            bn.bias.data.copy_(sl.bn[sl.d:])
            # ... and its running statistics, once ReplicaStep.rebind has moved ours into the exchange buffer (the module's
            # eval-mode encode, state_dict and checkpoints read the module's buffers)
            if sl.running_mean.data_ptr() != bn.running_mean.data_ptr():
                bn.running_mean.copy_(sl.running_mean)
                bn.running_var.copy_(sl.running_var)

    def sync_module(self):
        """before the attached module's state_dict is read (checkpoint.py): deferred updates settled, batch-norm parameters and
        running statistics copied, and num_batches_tracked moved on by the training-mode encode calls the slots counted on the
        host since the last call (`bn_calls`; torch's BatchNorm1d counts one per training-mode forward)"""
        self.flush()
        self._sync_module_batchnorms()
        for sl, bn in self.module_batchnorms:
            if sl.bn_calls:
                bn.num_batches_tracked += sl.bn_calls
                sl.bn_calls = 0

    def adopt_module(self):
        """after the attached module's state_dict was loaded: the slots' own copies of batch-norm parameters (and running
        statistics that no longer share the module's storage) follow the module"""
        for sl, bn in self.module_batchnorms:
            sl.bn[:sl.d].copy_(bn.weight.data)
            sl.bn[sl.d:].copy_(bn.bias.data)
            if sl.running_mean.data_ptr() != bn.running_mean.data_ptr():
                sl.running_mean.copy_(bn.running_mean)
                sl.running_var.copy_(bn.running_var)
            sl.bn_calls = 0
