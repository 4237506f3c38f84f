"""Token-pooled embedder: UnigramPoolingRelationEmbedder (openkge/model.py:715-796; its base
class is token_embedder.py's) over the HIP kernels of csrc/okge_pool.hip, and the training step that drives the fused
prefix-scoring path on rows computed from tokens.

Design: the pooled (and batch-normed) rows of one batch are written into the two virtual tables of virtual_tables.py (layout
and step skeleton); the fused step's dense row gradients then go back through batch-norm and the pooling into the token
tables' dense gradients, and Adagrad sweeps the token tables and the batch-norm parameters.  Every `_encode` call of the
reference (candidates, po rows, sp rows -- trainer.py:75-91) normalises with ITS OWN batch statistics and updates the
running statistics; that order is kept.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from typing import NamedTuple

import torch

from . import _native as N
from . import hotpath as H
from . import virtual_tables as VT
from .model import ComplexRelationScorer, DistmultRelationScorer, Models
from .token_embedder import BN_EPS, BN_MOMENTUM, TokenBasedRelationEmbedder, token_id_matrix  # noqa: F401  (token_id_matrix: re-exported)

POOLS = {"sum": 0, "mean": 1, "max": 2}


class TokenSlot:
    """One embedder slot (entity or relation): token table, token-id matrix, optional batch-norm, gradients."""

    bn_calls = 0      # training-mode batch-norm encode calls of a train step since VirtualTableStep.sync_module (host count)

    def __init__(self, W, token_ids, pool="sum", batchnorm=False, bn_weight=None, bn_bias=None, running=None, view=False):
        """running: (mean, var) to share (a module's buffers), None: fresh ones; view: a slot to encode with: no gradient,
        accumulator or touched-row buffers"""
        self.W, self.token_ids, self.pool = W, token_ids.to(torch.int32).contiguous(), pool
        d, dev = W.shape[1], W.device
        self.d = d
        # batch-norm parameters live in one flat buffer [weight | bias] so that one Adagrad launch covers them
        self.bn = None
        if batchnorm:
            self.bn = torch.empty(2 * d, dtype=torch.float32, device=dev)
            self.bn[:d] = torch.rand(d) if bn_weight is None else bn_weight        # init.uniform_(weight), model.py:613
            self.bn[d:] = 0.0 if bn_bias is None else bn_bias
            self.running_mean, self.running_var = running if running is not None else \
                (torch.zeros(d, dtype=torch.float32, device=dev), torch.ones(d, dtype=torch.float32, device=dev))
        if view:
            return
        if batchnorm:
            self.sum_bn = torch.zeros_like(self.bn)
        self.fresh_grads()
        self.dW = torch.zeros_like(W)
        self.sumW = torch.zeros_like(W)
        # touched-row map of dW for the optimizer sweep: the pooling backward stamps every row it writes, okge_adagrad_multi
        # skips the gradient rows that do not carry the current stamp (okge.h); the stamp moves on after every update
        self.touched = torch.zeros(W.shape[0], dtype=torch.uint8, device=dev) if d % 4 == 0 else None
        self.stamp = 1
        # optimizer steps every row has seen (TokenPooledTrainStep, decay_window > 1: deferred weight-decay-only updates)
        self.row_steps = torch.zeros(W.shape[0], dtype=torch.int32, device=dev) if d % 4 == 0 else None

    def next_stamp(self):
        self.stamp = self.stamp % 255 + 1

    def fresh_grads(self):
        """d_bn ([d weight | d bias]): a zeroed buffer of its own"""
        if self.bn is not None:
            self.d_bn = torch.zeros_like(self.bn)

    def optimizer_tensors(self):
        """the token table with the map the pooling backward stamps and the current stamp[, the batch-norm parameters]"""
        bn = [(self.bn, self.d_bn, self.sum_bn)] if self.bn is not None else []
        return [(self.W, self.dW, self.sumW, self.touched, self.stamp)] + bn

    @property
    def bn_weight(self):
        return None if self.bn is None else self.bn[:self.d]

    @property
    def bn_bias(self):
        return None if self.bn is None else self.bn[self.d:]

    def c(self):
        e = N.TokenEmbedder()
        e.W, e.token_ids = self.W.data_ptr(), self.token_ids.data_ptr()
        e.vocab, e.d, e.n_ids, e.max_len = self.W.shape[0], self.d, self.token_ids.shape[0], self.token_ids.shape[1]
        e.pool = POOLS[self.pool]
        if self.bn is not None:
            e.bn_weight, e.bn_bias = self.bn_weight.data_ptr(), self.bn_bias.data_ptr()
            e.bn_running_mean, e.bn_running_var = self.running_mean.data_ptr(), self.running_var.data_ptr()
            e.bn_eps, e.bn_momentum = BN_EPS, BN_MOMENTUM
        return e


class PoolEngine:
    """ctypes driver of okge_pool_encode / okge_pool_backward."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.lib = N.lib()
        self._ws, self._ws_bytes = None, 0
        self._state, self._state_bytes = None, 0
        # token-table scatter of the backward: "plan" = store-and-sum (bit-reproducible, okge.h) wherever it applies,
        # "atomics" = float atomics everywhere (the path max pooling and d % 4 != 0 always take)
        self.scatter = "plan"

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _workspace(self, n, d):
        need = int(self.lib.okge_pool_workspace_bytes(n, d))
        if need > self._ws_bytes:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws_bytes = need
        return self._ws

    def encode(self, slot: TokenSlot, ids, first_id, n, training, raw, out, saved):
        """raw / out: (n, d) row blocks (views into the virtual tables); saved: (4*d,) or None without batch-norm"""
        if n == 0:
            return
        ws = self._workspace(n, slot.d)
        e = slot.c()
        N.check(self.lib.okge_pool_encode(ctypes.byref(e), None if ids is None else ids.data_ptr(), int(first_id), int(n),
                                          int(training), raw.data_ptr(), out.data_ptr(), raw.stride(0),
                                          None if saved is None else saved.data_ptr(), ws.data_ptr(), self._ws_bytes,
                                          self._stream()), "okge_pool_encode")

    def backward(self, slot: TokenSlot, ids, first_id, n, raw, d_out, saved):
        if n == 0:
            return
        ws = self._workspace(n, slot.d)
        e = slot.c()
        bn = slot.bn is not None
        N.check(self.lib.okge_pool_backward(ctypes.byref(e), None if ids is None else ids.data_ptr(), int(first_id), int(n),
                                            raw.data_ptr(), d_out.data_ptr(), raw.stride(0),
                                            saved.data_ptr() if bn else None, slot.dW.data_ptr(),
                                            slot.d_bn[:slot.d].data_ptr() if bn else None,
                                            slot.d_bn[slot.d:].data_ptr() if bn else None, ws.data_ptr(), self._ws_bytes,
                                            self._stream()), "okge_pool_backward")

    # -- a batch of _encode calls in one go (okge_pool_encode_calls / okge_pool_backward_calls) ----------------------
    def _calls(self, calls, backward):
        """calls: [(slot, ids, first_id, n, raw, out_or_d_out, saved)] with n > 0 -> (ctypes array, keep-alive list)"""
        arr = (N.PoolCall * len(calls))()
        keep, need = [], 0
        for x, (slot, ids, first_id, n, raw, other, saved) in zip(arr, calls):
            e = slot.c()
            keep.append(e)
            x.e = ctypes.pointer(e)
            x.ids, x.first_id, x.n = None if ids is None else ids.data_ptr(), int(first_id), int(n)
            x.raw, x.ld = raw.data_ptr(), raw.stride(0)
            x.saved = None if saved is None else saved.data_ptr()
            if backward:
                x.d_out, x.dW = other.data_ptr(), slot.dW.data_ptr()
                if slot.bn is not None:
                    x.d_bn_weight, x.d_bn_bias = slot.d_bn[:slot.d].data_ptr(), slot.d_bn[slot.d:].data_ptr()
                if slot.touched is not None:
                    x.row_touched, x.touched_stamp = slot.touched.data_ptr(), int(slot.stamp)
            else:
                x.out = other.data_ptr()
            need += int(self.lib.okge_pool_workspace_bytes(int(n), slot.d))
        if backward and self.scatter_plan(calls):
            need = int(self.lib.okge_pool_backward_workspace_bytes(arr, len(calls)))
            state = int(self.lib.okge_pool_scatter_state_bytes(arr, len(calls)))
            if state > self._state_bytes:
                # zeroed ONCE: the kernels leave the state zero (okge.h); a graph capture must not allocate
                self._state = torch.zeros(state, dtype=torch.uint8, device=self.device)
                self._state_bytes = state
        if need > self._ws_bytes:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws_bytes = need
        return arr, keep

    def scatter_plan(self, calls):
        """store-and-sum scatter (bit-reproducible, okge.h) where it applies, unless self.scatter asks for the atomics"""
        return self.scatter != "atomics" and all(c[0].pool != "max" and c[0].d % 4 == 0 for c in calls)

    def encode_calls(self, calls, training):
        calls = [c for c in calls if c[3] > 0]
        if not calls:
            return
        arr, keep = self._calls(calls, False)
        N.check(self.lib.okge_pool_encode_calls(arr, len(calls), int(training), None if self._ws is None else self._ws.data_ptr(),
                                                self._ws_bytes, self._stream()), "okge_pool_encode_calls")
        del keep

    def catch_up_calls(self, calls, lazy, counters, lr, weight_decay, eps):
        """okge_pool_catch_up_calls: the token rows the calls name take their pending decay-only Adagrad steps (before the
        forward reads them).  calls: as encode_calls; lazy: hotpath.HotPath.lazy_tensors(...)"""
        calls = [c for c in calls if c[3] > 0]
        if not calls:
            return
        arr, keep = self._calls(calls, False)
        N.check(self.lib.okge_pool_catch_up_calls(arr, len(calls), lazy, len(lazy), counters.data_ptr(), float(lr), float(weight_decay),
                                                  float(eps), self._stream()), "okge_pool_catch_up_calls")
        del keep

    def backward_calls(self, calls):
        calls = [c for c in calls if c[3] > 0]
        if not calls:
            return
        arr, keep = self._calls(calls, True)
        plan = self.scatter_plan(calls)
        N.check(self.lib.okge_pool_backward_calls(arr, len(calls), None if self._ws is None else self._ws.data_ptr(), self._ws_bytes,
                                                  self._state.data_ptr() if plan else None, self._state_bytes if plan else 0,
                                                  self._stream()), "okge_pool_backward_calls")
        del keep


class EncodeCall(NamedTuple):
    """One of the five encode calls of a step (TokenPooledTrainStep._encode) with its views of the virtual tables: ids (int32,
    or None: the range from `first`), raw = the pooled rows, out = the finished rows (behind the batch-norm; `raw` itself
    without one), d_out = their gradients, saved = the call's batch-norm statistics (4 * d) or None."""
    slot: TokenSlot
    ids: object
    first: int
    n: int
    raw: torch.Tensor
    out: torch.Tensor
    d_out: torch.Tensor
    saved: object

    def forward(self):                    # as PoolEngine.encode_calls / catch_up_calls take it
        return self[:6] + self[7:]

    def backward(self):                   # as PoolEngine.backward_calls takes it
        return self[:5] + self[6:]


class TokenPooledTrainStep(VT.VirtualTableStep):
    """forward + loss + backward + Adagrad for UnigramPooling{Complex,Distmult}RelationModel
    (Trainer.compute_one_batch, trainer.py:181-257, over model.py:762-796)."""

    def __init__(self, entity: TokenSlot, relation: TokenSlot, scorer, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8,
                 label_smoothing=0.0, dropout=0.0, relation_dropout=None, seed=0, engine=None, decay_window=None, optimizer="adagrad",
                 betas=(0.9, 0.999), grad_clip=0.0):
        super().__init__(entity, relation, scorer, loss=loss, lr=lr, weight_decay=weight_decay, eps=eps,
                         label_smoothing=label_smoothing, dropout=dropout, relation_dropout=relation_dropout, seed=seed, engine=engine,
                         optimizer=optimizer, betas=betas, grad_clip=grad_clip)
        # optimizer="adam": every row's moments decay every step, so there is no decay-only update to defer -- the window is 1,
        # whatever the table size or OKGE_LAZY_DECAY; the sweep still skips the gradient rows the maps do not stamp
        if self.optimizer == "adam":
            if decay_window not in (None, 1):
                raise ValueError("decay_window (deferred weight decay) belongs to the Adagrad step: Adam moves every row every step")
            decay_window = 1
        # decay_window (OKGE_LAZY_DECAY; 1 = every row every step): the reference's Adagrad moves EVERY token row in
        # every step by its weight-decay term (utils/optim.py:139-160) -- 1 GB of read-modify-write at configs[4], 175 us of a
        # 0.78 ms step, for rows nothing reads.  With a window W > 1 a row no batch names takes its pending decay-only steps
        # later, all at once in registers (okge_adagrad_lazy, okge.h): when a batch names it (catch-up before the forward),
        # when its turn in the rotating 1/W sweep comes, or at flush().  Same operations, same order: after flush() the tables
        # are bit-identical to W = 1 (test_lazy_decay_is_bit_equal_to_the_eager_sweep).  CONTRACT: between steps, rows no
        # batch named may lag by up to W - 1 decay-only steps; everything in this package that reads the tables (evaluation,
        # state_tensors / checkpoints, the module's encode methods and state_dict) calls flush() first -- do the same before
        # reading .W / .sumW directly, and before DISCARDING a step object whose tables live on (its pending steps go with it).
        # Default: window 8 for token tables of 96 MB and more, 1 below -- the deferral trades the sweep's HBM time (0.7 us per MB of
        # table) for a catch-up launch and replay arithmetic that do not shrink with the table: at 45 MB it LOSES 40 us per step
        # (tools/soak_lazy.py), at configs[4]'s 256 MB it wins 130.
        if decay_window is None:
            env = os.environ.get("OKGE_LAZY_DECAY")
            big = (entity.W.numel() + relation.W.numel()) * 4 >= (96 << 20)
            decay_window = int(env) if env else (8 if big else 1)
        lazy_ok = all(sl.row_steps is not None and sl.touched is not None for sl in (entity, relation))
        self.decay_window = max(1, int(decay_window)) if lazy_ok else 1
        self._counters = torch.zeros(2, dtype=torch.int32, device=entity.W.device)      # [optimizer steps taken, scratch]
        self._pending = None              # (lr, weight_decay, eps) of the deferred steps; None: every row is current
        self.pool = PoolEngine(self.device)
        self.saved = torch.zeros((5, 4 * entity.d), device=self.device)      # batch-norm statistics of the five encode calls

    def state_tensors(self):
        self.flush()
        out = []
        for sl in (self.entity, self.relation):
            out += [sl.W, sl.dW, sl.sumW]
            if sl.bn is not None:
                out += [sl.bn, sl.d_bn, sl.sum_bn, sl.running_mean, sl.running_var]
        if self.decay_window > 1:         # (a caller that restores a snapshot restores the step counters with it)
            out += [self.entity.row_steps, self.relation.row_steps, self._counters]
        return out + self._optimizer_state()

    def _param_groups(self, every=False):
        """both token tables (with the maps the pooling backward stamps), then both slots' batch-norm parameters"""
        e, r = self.entity.optimizer_tensors(), self.relation.optimizer_tensors()
        return [e[0], r[0]] + e[1:] + r[1:]

    # -- deferred weight-decay-only updates (decay_window > 1) ---------------------------------------------------------
    def _hparams(self):
        return (float(self.lr), float(self.weight_decay), float(self.eps))

    def _lazy_tables(self):
        return [(sl.W, sl.dW, sl.sumW, sl.row_steps, sl.touched, sl.stamp) for sl in (self.entity, self.relation)]

    def flush(self):
        """every token row takes the decay-only steps it still owes: afterwards the tables are those of the eager sweep"""
        if self._pending is None:
            return
        lr, wd, eps = self._pending
        self.engine.adagrad_lazy(self._lazy_tables(), self._counters, self.decay_window, True, lr, wd, eps)
        self._pending = None

    def mark_pending(self):
        """a captured graph holding this step was replayed: rows may owe steps again (GraphedTrainStep)"""
        if self.decay_window > 1:
            self._pending = self._hparams()

    def _settle_hparams(self):
        """pending steps were taken with the lr / weight decay / eps of their time: flush before these change"""
        if self._pending is not None and self._pending != self._hparams():
            self.flush()

    # -- sharded.ReplicaStep protocol: gradients / running statistics as views into one flat exchange buffer ---------
    def grad_tensors(self):
        out = []
        for sl in (self.entity, self.relation):
            out.append(sl.dW)
            if sl.bn is not None:
                out.append(sl.d_bn)
        return out

    def stat_tensors(self):
        out = []
        for sl in (self.entity, self.relation):
            if sl.bn is not None:
                out += [sl.running_mean, sl.running_var]
        return out

    def sparse_grad_indices(self):
        """positions in grad_tensors() of the row-sparse gradients (the token tables')"""
        return [0, 2 if self.entity.bn is not None else 1]

    def sparse_grad_rows(self, batch: H.PrefixBatch):
        """token-table rows this batch's backward can touch (with repeats; row 0 = padding included, its gradient is 0):
        the token ids of the candidate + prefix entities, and of the prefix relations -- known from the ids alone"""
        dev = self.device
        cand = H._i32(batch.cand_ids, dev) if batch.cand_ids is not None else \
            torch.arange(batch.cand_first, batch.cand_first + batch.n_candidates, dtype=torch.int32, device=dev)
        ent = torch.cat([x for x in (cand, H._i32(batch.po_obj, dev), H._i32(batch.sp_subj, dev)) if x is not None]).long()
        rel = torch.cat([x for x in (H._i32(batch.po_rel, dev), H._i32(batch.sp_rel, dev)) if x is not None]).long()
        ie, ir = self.sparse_grad_indices()
        return [(ie, self.entity.token_ids.index_select(0, ent)), (ir, self.relation.token_ids.index_select(0, rel))]

    def rebind(self, grads, stats):
        gi, si = iter(grads), iter(stats)
        for sl in (self.entity, self.relation):
            sl.dW = next(gi)
            if sl.bn is not None:
                sl.d_bn = next(gi)
                sl.running_mean, sl.running_var = next(si), next(si)

    def _encode(self, batch: H.PrefixBatch, bufs):
        """catch-up of owed decay steps, then the pooling (+ batch-norm) forward of the five calls"""
        dev = self.device
        EV, EX, dEV, RV, RX, dRV = bufs
        ent, rel, pe = self.entity, self.relation, self.pool
        # the reference's encode order: candidates, (po rel, po obj), (sp subj, sp rel)   -- trainer.py:75-91
        calls = []
        for (relation, ids, first, rows), sv in zip(VT.encode_calls(batch), self.saved.unbind(0)):
            sl, X, V, dV = (rel, RX, RV, dRV) if relation else (ent, EX, EV, dEV)
            raw, bn = X[rows], sl.bn is not None
            calls.append(EncodeCall(sl, H._i32(ids, dev), first, rows.stop - rows.start, raw, V[rows] if bn else raw, dV[rows], sv if bn else None))
        # forward of all five calls: raw pooled rows -> EX / RX, batch-normed rows -> EV / RV (per-call statistics, running
        # statistics updated in this order)
        enc_calls = [c.forward() for c in calls]
        if self.decay_window > 1:
            # the token rows this batch names take the decay-only steps they owe before the forward reads them (always
            # launched: a captured graph must hold it; with nothing pending it reads the batch's step counters and ends)
            self._settle_hparams()
            lr, wd, eps = self._hparams()
            pe.catch_up_calls(enc_calls, self.engine.lazy_tensors(self._lazy_tables()), self._counters, lr, wd, eps)
        pe.encode_calls(enc_calls, True)
        for c in calls:
            if c.n > 0 and c.slot.bn is not None:
                c.slot.bn_calls += 1
        return calls

    def _backward(self, batch, bufs, calls):
        """dEV / dRV -> batch-norm and pooling backward of the five calls -> the slots' dW, d_bn ([d weight | d bias])"""
        self.pool.backward_calls([c.backward() for c in calls])

    def mark_sparse_rows(self, index, rows):
        """sharded.ReplicaStep wrote other replicas' gradient rows into a sparse gradient (grad_tensors()[index]): stamp them"""
        sl = self.entity if index == self.sparse_grad_indices()[0] else self.relation
        if sl.touched is not None:
            sl.touched.index_fill_(0, rows.reshape(-1).long(), sl.stamp)

    def optimizer_step(self):
        groups = self._param_groups()
        if self.decay_window > 1:
            # stamped rows: what they owe + this step with their gradient; one row in decay_window of the others: what they
            # owe + this step; batch-norm parameters: dense; the device step counter moves on (okge_adagrad_lazy)
            self._settle_hparams()
            lr, wd, eps = self._hparams()
            self._clip(groups)                        # (only stamped rows carry a gradient: the deferred rows are not its business)
            self.engine.adagrad_lazy(self._lazy_tables() + groups[2:], self._counters, self.decay_window, False, lr, wd, eps)
            self._pending = (lr, wd, eps)
            self._after_update()
            return
        # one launch: token tables (gradient rows the backward did not stamp are neither read nor cleared) + batch-norm parameters
        self._update(groups)
        self._after_update()

    def _after_update(self):
        for sl in (self.entity, self.relation):
            sl.next_stamp()
        self._sync_module_batchnorms()


# ------------------------------------------------------------------------------------------------------------------
# API-compatible model classes (inference protocol; training goes through TokenPooledTrainStep)
# ------------------------------------------------------------------------------------------------------------------
class UnigramPoolingRelationEmbedder(TokenBasedRelationEmbedder):
    """openkge/model.py:715-796.  Implemented: pool sum|mean|max, normalize None|'batchnorm', dropout; not implemented
    (raise): normalize='norm', activation, project_relation, sparse gradients.  Training: TokenPooledTrainStep (fused, own
    Adagrad) or trainer.AddLossModule (autograd bridge: any torch optimizer over the module's parameters)."""

    what, _train_step_class = "token-pooled", TokenPooledTrainStep

    def __init__(self, entity_slot_size, relation_slot_size, train_data, pool='sum', normalize=None, dropout=0.0,
                 entity_dropout=None, relation_dropout=None, sparse=False, init_std=0.01, activation=None,
                 project_relation=False, seed=0):
        super().__init__()
        self._refuse_unsupported(entity_slot_size, relation_slot_size, activation, project_relation, sparse)
        if normalize not in (None, 'batchnorm'):
            raise NotImplementedError(f"normalize={normalize!r}: the token-pooled embedder implements None and 'batchnorm'")
        self.pool = pool
        self._init_token_tables(train_data, entity_slot_size, normalize, init_std)
        self._init_state(dropout, entity_dropout, relation_dropout, seed)
        self._pool_engine = None

    # -- plumbing ----------------------------------------------------------------------------------------------
    def _pool(self):
        dev = self.entity_embedding.weight.device
        if self._pool_engine is None or self._pool_engine.device != dev:
            self._pool_engine = PoolEngine(dev)
        return self._pool_engine

    def _slot(self, relation, view=True):
        """a slot over the module's parameters (the table and the running statistics are the module's own tensors, the
        batch-norm parameters a copy); view: one to encode with"""
        emb, tok, _, bn = self._parts(relation)
        bn_args = () if bn is None else (True, bn.weight.data, bn.bias.data, (bn.running_mean, bn.running_var))
        return TokenSlot(emb.weight.data, tok, self.pool, *bn_args, view=view)

    def _encode(self, ids, relation, stream):
        """pool -> batch-norm (batch statistics in training mode, running statistics otherwise) -> dropout -> (n,1,d)"""
        eng = self.engine()
        self.flush_steps()
        ids = ids.reshape(-1).to(torch.int32).contiguous()
        n, d = ids.numel(), self.slot_size
        emb, tok, _, bn = self._parts(relation)
        p = (self.relation_dropout if relation else self.entity_dropout) if self.training else 0.0
        if torch.is_grad_enabled() and (emb.weight.requires_grad or (bn is not None and bn.weight.requires_grad)):
            # called with gradients enabled outside AddLossModule (a caller's own loss): the reference's op sequence in
            # torch (model.py:762-786; differentiable, the BatchNorm1d module keeps its own running statistics), dropout by
            # the Philox mask kernel (autograd_score.MaskRowsFn)
            from . import autograd_score as AG
            tokens = tok[ids.long()].long()
            embedded = emb(tokens)
            if self.pool == 'max':
                encoded, _ = embedded.max(dim=1)
            elif self.pool == 'mean':
                encoded = embedded.sum(dim=1) / ((tokens > 0).float().sum(1, keepdim=True) + 1e-12)
            else:
                encoded = embedded.sum(dim=1)
            if bn is not None:
                encoded = bn(encoded.contiguous())
            if p > 0:
                encoded = AG.MaskRowsFn.apply(encoded, eng, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
            return encoded.unsqueeze(1)
        slot = self._slot(relation)
        raw = torch.empty((n, d), device=ids.device)
        out = torch.empty_like(raw) if slot.bn is not None else raw
        saved = torch.empty(4 * d, device=ids.device) if slot.bn is not None else None
        self._pool().encode(slot, ids, 0, n, self.training, raw, out, saved)
        if p > 0:
            out = eng.encode_rows(out, None, 0, n, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
        return out.unsqueeze(1)

    def precompute_embeddings_from_tokens(self):
        """model.py:670-712, each table in one encode call"""
        if self.entity_embedding_from_tokens is None:
            super().train(False)                       # the reference calls self.eval() here and stays in eval mode
            dev = self.entity_embedding.weight.device
            ar = lambda n: torch.arange(n, dtype=torch.int32, device=dev)      # noqa: E731
            with torch.no_grad():                      # model.py:682: the precomputed tables carry no graph
                self.entity_embedding_from_tokens = self._encode(ar(self.train_data.entities_size), False, H.STREAM_CAND).squeeze(1)
                self.relations_embedding_from_tokens = self._encode(ar(self.train_data.relations_size), True, H.STREAM_SP_REL).squeeze(1)

    # -- the training bridges (TokenBasedRelationEmbedder) ---------------------------------------------------------------
    def _train_slots(self):
        return [self._slot(False, view=False), self._slot(True, view=False)]

    def autograd_step(self, loss, label_smoothing):
        """the cached TokenPooledTrainStep behind AddLossModule: shares the module's parameters; its optimizer is NOT used
        (the caller's torch optimizer steps the module parameters: it moves every row every step, so decay_window = 1)"""
        self.flush_steps()
        return self._refresh_autograd_step(self._cached_autograd_step(loss, label_smoothing, self._train_slots, decay_window=1))

    def autograd_params_and_grads(self, st):
        params, grads = [self.entity_embedding.weight, self.relation_embedding.weight], [st.entity.dW, st.relation.dW]
        for sl, bn in ((st.entity, self.entity_batchnorm), (st.relation, self.relation_batchnorm)):
            if bn is not None:
                params += [bn.weight, bn.bias]
                grads += [sl.d_bn[:sl.d], sl.d_bn[sl.d:]]
        return params, grads

    def _state_segments(self, sl, relation):
        """optimizer_params_and_state: the token table, then the batch-norm's [weight | bias]"""
        emb, tok, _, bn = self._parts(relation)
        out = [(emb.weight, (sl.W, sl.sumW), 0)]
        if bn is not None:
            out += [(bn.weight, (sl.bn, sl.sum_bn), 0), (bn.bias, (sl.bn, sl.sum_bn), sl.d)]
        return out

    def train_step(self, *args, **kwargs):
        """TokenBasedRelationEmbedder.train_step.  Token rows no batch named may owe decay-only Adagrad steps
        (TokenPooledTrainStep.decay_window): an earlier driver (another epoch's learning rate, ...) settles them before this one
        is built, and the module keeps a weak reference to every driver, so that everything that reads the parameters
        (flush_steps(): _encode, state_dict) settles them first."""
        self.flush_steps()
        st = super().train_step(*args, **kwargs)
        self._steps = [r for r in self._steps if r() is not None] + [weakref.ref(st)]
        return st


class UnigramPoolingComplexRelationModel(ComplexRelationScorer, UnigramPoolingRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


class UnigramPoolingDistmultRelationModel(DistmultRelationScorer, UnigramPoolingRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


# registered like the reference's (model.py:1052-1066): getattr(Models, args["model"])
Models.UnigramPoolingComplexRelationModel = UnigramPoolingComplexRelationModel
Models.UnigramPoolingDistmultRelationModel = UnigramPoolingDistmultRelationModel
