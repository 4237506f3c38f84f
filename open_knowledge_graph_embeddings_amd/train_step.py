"""One training step of the hot path, as `Trainer.compute_one_batch(training=True)` drives it in the
reference (openkge/trainer.py:181-257): forward + loss + backward + dense Adagrad on both tables.

All arithmetic is in libokge_hip.so; this class only owns the buffers (tables, dense gradients, Adagrad
accumulators) and sequences the C-ABI calls on the current stream.  No host synchronisation per step.
"""
from __future__ import annotations

import torch

from . import _native as N
from . import hotpath as H
from .step_optim import refuse_single_device

ENTITY_KEY, RELATION_KEY = "entity_embedding.weight", "relation_embedding.weight"


class TableState:
    """What FusedTrainStep holds for ONE of its two tables.  Plain storage: the step's methods run over both records, or over
    the trained ones.  `name`: what `freeze` calls the table; `index`: its parameter index in the reference's optimizer; `key`:
    its state_dict key.  A field the step's configuration does not use -- and everything but `param` and an Adagrad `sum` of
    a frozen table -- is None."""
    __slots__ = ("name", "index", "key", "param", "grad", "sum", "exp_avg", "exp_avg_sq", "adam_state", "row_steps")

    def __init__(self, name, index, key, param):
        self.name, self.index, self.key, self.param = name, index, key, param
        self.grad = None                                     # dense .grad
        self.sum = None                                      # Adagrad state 'sum'
        self.exp_avg = self.exp_avg_sq = None                # Adam state
        self.adam_state = None                               # HotPath.adam_state: the device step count
        self.row_steps = None                                # decay_window: optimizer steps every row has seen


class FusedTrainStep:
    def __init__(self, E: torch.Tensor, R: torch.Tensor, scorer: str, loss: str = "bce", lr: float = 0.3,
                 weight_decay: float = 1e-10, eps: float = 1e-8, label_smoothing: float = 0.0,
                 input_dropout: float = 0.0, relation_input_dropout: float = 0.0, seed: int = 0, engine=None,
                 grad_clip: float = 0.0, accumulate: int = 1, sparse: bool = False, decay_window=None,
                 l2_reg: float = 0.0, l2_reg_dropout: float = 0.0, l2_reg_per_direction: bool = False,
                 optimizer: str = "adagrad", betas=(0.9, 0.999), deterministic: bool = False, freeze=None):
        """Defaults follow config/fb15k237/fb15k237-complex-kge.yaml and the optimizer OptimRegime actually
        builds (utils/optim.py:29,139-160): Adagrad(lr, weight_decay=1e-10, eps=1e-8 leaked from Adam).

        sparse (model_config.sparse, model.py:390-391): gradients stay in occurrence rows and only the table rows a batch
        names are updated (okge_adagrad_rows) -- no dense dE / dR, nothing per step that grows with the tables.  Needs
        weight_decay = 0, as torch's sparse Adagrad does; no clipping (torch cannot clip sparse gradients), no accumulation.

        decay_window (sparse only; None: off): the row-sparse step WITH the reference's weight decay.  Dense Adagrad moves
        every row every step by its decay term; such a decay-only update depends on the row alone, so a row no batch names takes
        it later, all pending steps at once in registers (okge_rows_catch_up / okge_adagrad_rows_decay, okge.h): when a batch
        names it (catch-up before the forward), when its turn in the rotating 1 / decay_window sweep comes, or at flush().  After
        flush() tables and accumulators are bit-identical to the dense step's wherever that step's atomics are order-free.
        CONTRACT: between steps, rows no batch named may lag by up to decay_window - 1 decay-only steps -- call flush() before
        reading .E / .sumE / .R / .sumR or handing them to an evaluator (state_tensors() and the checkpoint writer do), and
        before discarding a step object whose tables live on.  Needs d % 4 == 0.

        l2_reg (LookupBaseRelationEmbedder's keyword, model.py:444-453, :471-479; 0: off, nothing is launched): the N3
        regulariser as the reference spells it -- l2_reg * sum |x|^3 over the rows every _encode call of the batch returns,
        after dropout -- added to each batch's gradients before clipping (okge_n3_forward_backward, issued behind the step's own
        call).  `reg_out` (device double[1], beside `loss_out`) receives the term's value, the Trainer's `hook`; the loss
        excludes it.  l2_reg_dropout: the embedder's `dropout`, by which the reference divides the rows before the cube when it
        is > 0 (the probability; a divisor only, this step applies input_dropout).  l2_reg_per_direction: the candidate block
        counts once per direction present (batch_shared_entities None, trainer.py:86-87) instead of once (a shared list).

        optimizer ("adagrad", the default: the object described above; or "adam", `optimization_config.optimizer: Adam`,
        utils/optim.py:143-145): torch.optim.Adam(lr, betas, eps, weight_decay) with coupled weight decay and no amsgrad
        (okge_adam_step).  The accumulators sumE / sumR give way to the moments mE / vE / mR / vR and one device state per table
        (adam_stateE / adam_stateR, int32[4], [0] = t: optimizer steps taken, counted on the device so that a captured graph
        replays it; `adam_t` reads it back).  Works with the dense and the wide step, accumulate, grad_clip and l2_reg.  With
        sparse=True it is torch.optim.SparseAdam on the occurrence rows (okge_adam_rows), which has no weight decay:
        weight_decay != 0 and decay_window raise ValueError.  `betas` is read by Adam only.

        deterministic (False: the step above, launch for launch): dense gradients with the ORDER of every row's additions fixed
        (okge.h, okge_rows_to_dense).  forward_backward runs the occurrence-row call (OKGE_TRAIN_ROW_GRADS: every gradient
        contribution stored once, no atomics) with the masks of the default step, then writes each table row's sequential fp32
        sum in ascending occurrence position into dE / dR -- stored on the first micro-batch of an accumulation window, continued
        from the row's value on the later ones -- and the dense tail runs unchanged: grad_clip (its norm stays in `grad_norm`,
        device double[1]), accumulate, dense Adagrad / Adam with weight_decay, GraphedTrainStep, checkpoints.  Two runs from one
        state and seed are bit-identical on ANY batch; at weight_decay = 0 the Adagrad step is bit-equal to sparse=True, and at
        weight_decay > 0 to sparse=True with a decay_window after flush().  Costs the (N + 2 B) x d occurrence-row traffic and
        a key sort per step.  Refused: sparse=True (already reproducible), l2_reg > 0 (the N3 kernel's gradient rows go through
        float atomics), slot sizes above 512 and N + n_po + n_sp > 2^20 (the occurrence-row call's limits).

        freeze (None: the step above, launch for launch; "entities" or "relations": the reference's resume_freeze,
        trainer.py:532-536 -- requires_grad = False on that table): the frozen table, its gradient and its optimizer state are
        never touched -- a step constructed fresh does not even allocate dE / sumE / mE / vE / adam_stateE (or their R
        counterparts): they are None, unless a checkpoint brought an Adagrad `sum` along, which is kept as it came.  The call
        passes OKGE_TRAIN_FREEZE_ENTITIES / _RELATIONS (okge.h; with "entities" the tile kernels run without their
        candidate-gradient product), the optimizer sweeps the trained table alone, and grad_clip clips -- `grad_norm` (device
        double[1]) reports -- the norm of the trained table's gradient alone, as clip_grad_norm_ over parameters without .grad
        does.  Works with accumulate, the wide path, Adam, GraphedTrainStep and checkpoints.  A zero gradient is not a freeze:
        weight decay and eps still move the table ("The untouched slot").  Refused: sparse=True, deterministic=True
        and l2_reg > 0 (NotImplementedError)."""
        N.refuse_bias_scorer(scorer, type(self).__name__)
        H.freeze_flag(freeze)                 # (ValueError for anything but None / "entities" / "relations")
        self.freeze = freeze
        if freeze is not None:
            if sparse:
                raise NotImplementedError(f"FusedTrainStep(freeze={freeze!r}, sparse=True): the row-sparse step trains both tables; "
                                          f"drop sparse=True (dense gradients), or freeze")
            if deterministic:
                raise NotImplementedError(f"FusedTrainStep(freeze={freeze!r}, deterministic=True): the occurrence-row call trains both "
                                          f"tables; drop deterministic=True, or freeze")
            if float(l2_reg or 0.0) > 0:
                raise NotImplementedError(f"FusedTrainStep(freeze={freeze!r}, l2_reg={l2_reg}): the N3 kernel adds to both tables' "
                                          f"gradients; drop l2_reg (l2_reg=0), or freeze")
        self.optimizer = str(optimizer).lower()
        if self.optimizer not in ("adagrad", "adam"):
            raise ValueError(f"optimizer {optimizer!r}: 'adagrad' or 'adam'")
        self.betas = (float(betas[0]), float(betas[1]))
        if self.optimizer == "adam":
            if not (0.0 <= self.betas[0] < 1.0 and 0.0 <= self.betas[1] < 1.0):
                raise ValueError(f"Invalid beta parameters: {betas}")
            if decay_window is not None:
                raise ValueError("decay_window (deferred weight decay) belongs to the Adagrad step: SparseAdam has no weight decay")
            if sparse and weight_decay != 0:
                raise ValueError("weight_decay option is not compatible with sparse gradients (SparseAdam has no weight decay)")
        self.sparse = bool(sparse)
        self.deterministic = bool(deterministic)
        self._row_grads = self.sparse or self.deterministic      # the step's call leaves occurrence rows (OKGE_TRAIN_ROW_GRADS)
        if self.deterministic:
            if self.sparse:
                raise ValueError("FusedTrainStep(deterministic=True, sparse=True): the row-sparse step is already bit-reproducible; "
                                 "use sparse=True alone, or deterministic=True alone for dense gradients")
            if float(l2_reg or 0.0) > 0:
                raise NotImplementedError("FusedTrainStep(deterministic=True): the N3 regulariser adds its gradient rows with float "
                                          "atomics; train with l2_reg=0, or with deterministic=False")
            if E.shape[1] > H.TILE_MAX_SLOT:
                raise NotImplementedError(f"FusedTrainStep(deterministic=True): the occurrence-row call stops at slot size "
                                          f"{H.TILE_MAX_SLOT}; slot sizes up to {H.WIDE_MAX_SLOT} train with deterministic=False")
        self.decay_window = None if decay_window is None else int(decay_window)
        if self.decay_window is not None and (not self.sparse or self.decay_window < 1):
            raise ValueError("decay_window (deferred weight decay) belongs to the sparse step and is >= 1")
        if E.shape[1] > H.WIDE_MAX_SLOT:
            raise NotImplementedError(f"FusedTrainStep: slot sizes above {H.WIDE_MAX_SLOT}")
        if self.sparse and E.shape[1] > H.TILE_MAX_SLOT:
            raise NotImplementedError(f"FusedTrainStep(sparse=True): the row-sparse step stops at slot size {H.TILE_MAX_SLOT}; slot "
                                      f"sizes up to {H.WIDE_MAX_SLOT} train with dense gradients (sparse=False)")
        if self.sparse:
            if weight_decay != 0 and self.decay_window is None:
                raise ValueError("weight_decay option is not compatible with sparse gradients")
            if self.decay_window is not None and E.shape[1] % 4:
                raise NotImplementedError("FusedTrainStep(sparse=True, decay_window=...): the deferred decay works on 16-byte "
                                          "column groups, the slot size must be a multiple of 4")
            if float(grad_clip or 0.0) > 0 or int(accumulate) > 1:
                raise NotImplementedError("FusedTrainStep(sparse=True): grad_clip and accumulate need dense gradients "
                                          "(torch.nn.utils.clip_grad_norm_ refuses sparse gradients)")
        self.ent, self.rel = TableState("entities", 0, ENTITY_KEY, E), TableState("relations", 1, RELATION_KEY, R)
        self.tables = (self.ent, self.rel)
        self.scorer, self.loss = scorer, loss
        self.lr, self.weight_decay, self.eps = lr, weight_decay, eps
        self.label_smoothing = label_smoothing
        self.input_dropout, self.relation_input_dropout = input_dropout, relation_input_dropout
        self.seed = seed
        self.engine = engine or H.HotPath(E.device)
        self._call = H.PrefixCall()       # persistent argument structs of the per-step call (_fast_forward_backward)
        self._rows = {}
        self._allocate()
        if self.decay_window is not None:
            # deferred weight decay: optimizer steps every row has seen, [steps taken, scratch] on the device (a captured graph
            # replays them), and the (lr, weight_decay, eps) of the steps rows still owe -- None: every row is current
            for t in self.tables:
                t.row_steps = torch.zeros(t.param.shape[0], dtype=torch.int32, device=t.param.device)
            self._counters = torch.zeros(2, dtype=torch.int32, device=E.device)
        self._pending = None
        self.steps = 0
        self.step_dev = None              # device step counter, attached by GraphedTrainStep
        self._grads_zero = True           # fresh buffers; kept true by the zero_grad fused into Adagrad
        self._dE_stale = False            # dE holds last step's values (they get overwritten, not accumulated)
        self.loss_out = torch.zeros(1, dtype=torch.float64, device=E.device)
        self.l2_reg, self.l2_reg_dropout = float(l2_reg or 0.0), float(l2_reg_dropout or 0.0)
        self.l2_reg_per_direction = bool(l2_reg_per_direction)
        if self.l2_reg < 0 or self.l2_reg_dropout < 0:
            raise ValueError("l2_reg and l2_reg_dropout are non-negative")
        self.reg_out = torch.zeros(1, dtype=torch.float64, device=E.device)   # value of the l2_reg term of the last batch
        # trainer.py:229-244: gradients of `accumulate` consecutive batches are summed before one optimizer step
        # (batch_size_for_backward = accumulate x batch_size), clipped to `grad_clip` (global 2-norm) if > 0
        self.grad_clip, self.accumulate = float(grad_clip or 0.0), max(1, int(accumulate))
        self._accumulated = 0
        # deterministic: the global 2-norm of the last clipped gradient (okge_clip_grad_norm: fixed grid, fixed reduction tree)
        # (and of a frozen step's: the norm of the trained table's gradient alone)
        self.grad_norm = torch.zeros(1, dtype=torch.float64, device=E.device) \
            if (self.deterministic or freeze is not None) and self.grad_clip > 0 else None

    def _allocate(self):
        """zeros for the gradient and the optimizer state a trained table lacks (dense .grad unless model_config.sparse: the sparse
        step keeps per-shape occurrence-row buffers instead, _row_buffers); a frozen table keeps nothing but an Adagrad `sum`"""
        for t in self.tables:
            if t.name == self.freeze:
                t.grad = t.exp_avg = t.exp_avg_sq = t.adam_state = None
                continue
            zeros = lambda x, t=t: torch.zeros_like(t.param) if x is None else x      # noqa: E731
            if not self.sparse:
                t.grad = zeros(t.grad)
            if self.optimizer == "adam":  # Adam state 'exp_avg' / 'exp_avg_sq' (init 0) and the device step count
                t.exp_avg, t.exp_avg_sq = zeros(t.exp_avg), zeros(t.exp_avg_sq)
                if t.adam_state is None:  # (a table that trains again takes the count of the one that never stopped)
                    other = self.tables[1 - t.index].adam_state
                    t.adam_state = H.HotPath.adam_state(t.param.device) if other is None else other.clone()
            else:
                t.sum = zeros(t.sum)      # Adagrad state 'sum' (init 0)
        self.trained = tuple(t for t in self.tables if t.name != self.freeze)

    def set_freeze(self, freeze):
        """Freeze a table of a step that exists (checkpoint.load_reference_checkpoint(freeze_param=...), the reference's
        resume_freeze), or train both again (None).  The frozen table's gradient buffer and Adam state are dropped; an Adagrad
        `sum` is kept untouched, as torch keeps it for a parameter without .grad.  The refusals of the constructor hold."""
        H.freeze_flag(freeze)
        if freeze is not None and (self.sparse or self.deterministic or self.l2_reg > 0):
            raise NotImplementedError(f"FusedTrainStep.set_freeze({freeze!r}): not with sparse=True, deterministic=True or l2_reg > 0 "
                                      f"(they train both tables); drop them, or freeze")
        if self._accumulated:
            raise RuntimeError("set_freeze inside an accumulation window: the gradients of earlier micro-batches would be lost")
        self.freeze = freeze
        self._allocate()
        self._grads_zero, self._dE_stale = True, False
        for t in self.trained:
            t.grad.zero_()
        if (self.deterministic or freeze is not None) and self.grad_clip > 0 and self.grad_norm is None:
            self.grad_norm = torch.zeros(1, dtype=torch.float64, device=self.ent.param.device)

    def state_tensors(self):
        """every tensor a step mutates (GraphedTrainStep snapshots them around its warm-up, by position): the trained tables,
        their dense gradients, their optimizer state -- a frozen table and what it holds are not among them"""
        tr = self.trained
        out = [t.param for t in tr] + [t.grad for t in tr if t.grad is not None]    # (the row buffers are written whole every step)
        if self.optimizer == "adam":       # (the device states with them: restoring a snapshot restores t)
            return out + [m for t in tr for m in (t.exp_avg, t.exp_avg_sq)] + [t.adam_state for t in tr]
        if self.decay_window is None:
            return out + [t.sum for t in tr]
        self.flush()                       # (a caller that restores a snapshot restores the step counters with it)
        return out + [t.sum for t in tr] + [t.row_steps for t in tr] + [self._counters]

    @property
    def adam_t(self):
        """optimizer steps the Adam state has taken (read back from the device: synchronises)"""
        return int(self.trained[0].adam_state[0].item())

    def set_adam_t(self, t):
        """the trained tables' device step counts (a loaded checkpoint, a reset)"""
        for st in (tab.adam_state for tab in self.trained):     # (a frozen table has none)
            st.zero_()
            st[0] = int(t)

    # -- sparse step with deferred weight decay (decay_window) ----------------------------------------------------------
    def _hparams(self):
        return (float(self.lr), float(self.weight_decay), float(self.eps))

    def flush(self):
        """every row of both tables takes the decay-only steps it still owes: afterwards the tables are the dense step's"""
        if self._pending is None:
            return
        lr, wd, eps = self._pending
        # (no row is stamped in a flush, so the gradient operand is never read: the accumulator stands in)
        self.engine.adagrad_lazy([(t.param, t.sum, t.sum, t.row_steps) for t in self.tables], self._counters, self.decay_window, True,
                                 lr, wd, eps)
        self._pending = None

    def mark_pending(self):
        """a captured graph holding this step was replayed: rows may owe steps again (GraphedTrainStep)"""
        if self.decay_window is not None and self.decay_window > 1:
            self._pending = self._hparams()

    def _settle_hparams(self):
        """pending steps were taken with the lr / weight decay / eps of their time: flush before these change"""
        if self._pending is not None and self._pending != self._hparams():
            self.flush()

    # -- sparse step: occurrence rows ------------------------------------------------------------------------------------
    def _row_buffers(self, batch: H.PrefixBatch):
        """per shape (N, n_po, n_sp): gradient rows gE (N + B, d) / gR (B, d) and the occurrence ids idE = [candidate ids |
        po_obj | sp_subj], idR = [po_rel | sp_rel] -- persistent storage, so a captured graph refills and reuses it"""
        n, n_po, n_sp = batch.n_candidates, batch.n_po, batch.n_sp
        key = (n, n_po, n_sp)
        rb = self._rows.get(key)
        if rb is None:
            dev, d, B = self.ent.param.device, self.ent.param.shape[1], n_po + n_sp
            rb = self._rows[key] = dict(gE=torch.empty((n + B, d), dtype=torch.float32, device=dev),
                                        gR=torch.empty((B, d), dtype=torch.float32, device=dev),
                                        idE=torch.empty(n + B, dtype=torch.int32, device=dev),
                                        idR=torch.empty(B, dtype=torch.int32, device=dev))
        return rb

    def _occurrences(self, rb):
        """(record, occurrence ids, gradient rows) of both tables in the row buffers rb"""
        return (self.ent, rb["idE"], rb["gE"]), (self.rel, rb["idR"], rb["gR"])

    def _covers_all_rows(self, batch: H.PrefixBatch):
        """1-vs-all: the candidate range is every row from cand_first on, so the step overwrites all of dE it uses"""
        return batch.cand_ids is None and batch.cand_first + batch.n_cand == self.ent.param.shape[0]

    def _set_dropout(self, batch: H.PrefixBatch):
        batch.set_dropout(H.dropout_specs(self.input_dropout, self.relation_input_dropout, self.seed, self.steps, self.step_dev))

    def _fast_forward_backward(self, batch: H.PrefixBatch, normalizer, dE, dR):
        """same call as HotPath.forward_backward for int32 device tensors (what the batch producer emits), issued from the
        step's persistent argument structs (H.PrefixCall)"""
        if H.VALIDATE:
            H.validate_ids(batch, self.ent.param.shape[0], self.rel.param.shape[0])
        call = self._call
        call.fill_tables(self.ent.param, self.rel.param, self.scorer, self.engine.device)
        call.fill_ids(batch.po_rel, batch.po_obj, batch.sp_subj, batch.sp_rel, batch.cand_ids, batch.cand_first, batch.n_cand,
                      batch.pos_row, batch.pos_col)
        call.fill_dropout(self.input_dropout, self.relation_input_dropout, self.seed, self.steps, self.step_dev)
        flags = H.train_flags(row_grads=True) if self._row_grads else \
            H.train_flags(grads_zero=self._grads_zero, unique_candidates=batch.cand_unique, freeze=self.freeze)
        return call.train(self.engine, self.loss, self.label_smoothing, normalizer, flags, self.loss_out, dE, dR)

    def _plain(self, batch: H.PrefixBatch):
        """int32 contiguous tensors ON THE ENGINE'S DEVICE everywhere and no replayed masks: nothing for the generic path
        to convert (a host tensor's data_ptr handed to a kernel would be a GPU fault)"""
        dev = self.ent.param.device
        for x in (batch.po_rel, batch.po_obj, batch.sp_subj, batch.sp_rel, batch.pos_row, batch.pos_col, batch.cand_ids):
            if x is not None and (x.dtype != torch.int32 or not x.is_contiguous() or x.dim() != 1 or x.device != dev):
                return False
        return batch.pos_row is not None and batch.cand_table is None

    def _regularise(self, batch: H.PrefixBatch, normalizer, fast, dE, dR):
        """the l2_reg term of this batch, added to the gradients the step's call just left (same masks: same seed, streams, step;
        `fast`: the structs that call was issued from still hold them)"""
        coef = H.n3_coef(self.l2_reg, self.l2_reg_dropout)
        passes = (int(batch.n_po > 0) + int(batch.n_sp > 0)) if self.l2_reg_per_direction else 1
        if fast:
            flags = H.train_flags(unique_candidates=batch.cand_unique, row_grads=self.sparse)
            self._call.n3(self.engine, coef, passes, normalizer, flags, self.reg_out, dE, dR)
        else:
            self.engine.n3_forward_backward(self.ent.param, self.rel.param, self.scorer, batch, dE, dR, coef, cand_passes=passes, normalizer=normalizer,
                                            reg_out=self.reg_out, row_grads=self.sparse)

    def _fill_row_buffers(self, batch: H.PrefixBatch):
        """this batch's row buffers (the step's current ones from here on) with its occurrence ids written"""
        rb = self._row_buffers(batch)
        H.occurrence_ids(self.ent.param.device, batch.cand_ids, batch.cand_first, batch.n_candidates, batch.po_obj, batch.sp_subj,
                         batch.po_rel, batch.sp_rel, out=(rb["idE"], rb["idR"]))
        self._cur_rows = rb
        return rb

    def _issue(self, batch: H.PrefixBatch, normalizer, dE, dR):
        """the step's call into dE / dR -> (loss, fast); fast: it went out from the step's persistent structs, which still hold
        the batch and its masks (_regularise), and not through the engine's converting entry point"""
        fast = isinstance(self.engine, H.HotPath) and self._plain(batch)
        if fast:
            return self._fast_forward_backward(batch, normalizer, dE, dR), True
        self._set_dropout(batch)
        how = dict(row_grads=True) if self._row_grads else dict(grads_zero=self._grads_zero)
        if self.freeze is not None:
            how["freeze"] = self.freeze
        loss = self.engine.forward_backward(self.ent.param, self.rel.param, self.scorer, batch, dE, dR, loss=self.loss,
                                            label_smoothing=self.label_smoothing, normalizer=normalizer, loss_out=self.loss_out, **how)
        return loss, False

    def forward_backward(self, batch: H.PrefixBatch, normalizer=None):
        """trainer.py:206-234.  Returns the summed loss (device double[1], valid after stream sync)."""
        if self.deterministic:                # (a method of its own: the default step is host-bound, its path stays short)
            return self._deterministic_forward_backward(batch, normalizer)
        if self.sparse:
            rb = self._fill_row_buffers(batch)
            self._last_full = False
            if self.decay_window is not None:      # the rows this batch names take what they owe BEFORE the gather reads them
                self._settle_hparams()
                lr, wd, eps = self._hparams()
                self.engine.rows_catch_up([(t.param, t.sum, ids, t.row_steps) for t, ids, _ in self._occurrences(rb)], self._counters,
                                          lr, wd, eps)
            dE, dR = rb["gE"], rb["gR"]
        else:
            dE, dR = self.ent.grad, self.rel.grad
            if dE is not None and self._dE_stale and not (self._grads_zero and self._covers_all_rows(batch)):
                dE.zero_()                # a sampled candidate list leaves rows untouched: they must read as zero
                self._dE_stale = False
            self._last_full = self._covers_all_rows(batch)
        loss, fast = self._issue(batch, normalizer, dE, dR)
        if self.l2_reg > 0:
            self._regularise(batch, normalizer, fast, dE, dR)
        return loss

    def _deterministic_forward_backward(self, batch: H.PrefixBatch, normalizer):
        """the occurrence-row call into the per-shape row buffers, then okge_rows_to_dense into dE / dR (class docstring)"""
        if batch.n_candidates + batch.B > H.ROWS_MAX_N:            # (before anything is launched or allocated)
            raise N.OkgeError(f"okge_rows_to_dense takes up to 2^20 occurrence rows per tensor: this batch has "
                              f"{batch.n_candidates} + {batch.B}; train it with deterministic=False")
        rb = self._fill_row_buffers(batch)
        # a store names -- and so overwrites -- every row of dE only when the candidate range is the whole table from row 0
        names_all = self._covers_all_rows(batch) and batch.cand_first == 0
        if self._dE_stale and not (self._grads_zero and names_all):
            self.ent.grad.zero_()         # rows this batch does not name must read as zero
            self._dE_stale = False
        self._last_full = names_all
        loss, _ = self._issue(batch, normalizer, rb["gE"], rb["gR"])
        # cleared tables (a fresh window): the named rows are stored; later micro-batches continue each row's chain
        self.engine.rows_to_dense([(t.grad, ids, g) for t, ids, g in self._occurrences(rb)], accumulate=not self._grads_zero)
        return loss

    def optimizer_step(self, lazy_zero=False):
        """trainer.py:240-244: optimizer.step() then zero_grad() -- one sweep per table.  lazy_zero (used by step()
        after a 1-vs-all batch): the entity gradient is not cleared here because the next 1-vs-all step overwrites
        every row it uses; it is cleared on demand if a sampled candidate list comes next.
        Sparse step: torch's sparse Adagrad on the occurrence rows of the last forward_backward -- nothing to clear; with a
        decay_window the same rows take the dense step's expression, then the due slice of the deferred decay-only steps.
        A frozen table: the same update rule and fused zero_grad on the trained table alone (okge_adagrad_step / okge_adam_step
        with one tensor); the frozen one takes no decay and has no state to move."""
        trained = self.trained
        keep = bool(lazy_zero) and trained[0] is self.ent      # only the entity gradient can be left for the next step to overwrite
        if self.sparse:                   # (trains both tables)
            rows = self._occurrences(self._cur_rows)
            if self.optimizer == "adam":  # torch.optim.SparseAdam on the occurrence rows
                self.engine.adam_rows([(t.param, t.exp_avg, t.exp_avg_sq, t.adam_state, ids, g) for t, ids, g in rows],
                                      self.lr, self.betas, self.eps)
            elif self.decay_window is not None:
                self._settle_hparams()
                lr, wd, eps = self._hparams()
                self.engine.adagrad_rows_decay([(t.param, t.sum, ids, g, t.row_steps) for t, ids, g in rows], self._counters,
                                               self.decay_window, lr, wd, eps)
                if self.decay_window > 1:
                    self._pending = (lr, wd, eps)
            else:
                (e, ide, ge), (r, idr, gr) = rows
                self.engine.adagrad_rows(e.param, e.sum, ide, ge, self.lr, self.eps, second=(r.param, r.sum, idr, gr))
            return
        if self.optimizer == "adam":      # zero_grad: 0 none, 1 all, 2 the second tensor alone
            self.engine.adam([(t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.adam_state) for t in trained], self.lr, self.betas, self.eps,
                             self.weight_decay, zero_grad=(2 if len(trained) == 2 else 0) if keep else 1)
        elif len(trained) == 2:
            e, r = trained
            self.engine.adagrad2(e.param, e.grad, e.sum, r.param, r.grad, r.sum, self.lr, self.weight_decay, self.eps,
                                 zero_grad=2 if keep else 1)
        else:
            t, = trained
            self.engine.adagrad(t.param, t.grad, t.sum, self.lr, self.weight_decay, self.eps, zero_grad=not keep)
        self._dE_stale = keep

    def step(self, batch: H.PrefixBatch, normalizer=None):
        """forward + loss + backward; every `accumulate`-th call also clips (grad_clip > 0) and takes the Adagrad step"""
        self.steps += 1
        loss = self.forward_backward(batch, normalizer)
        self._grads_zero = False
        self._accumulated += 1
        if self._accumulated < self.accumulate:
            return loss                      # trainer.py:233-234, 246-248: no optimizer step yet, gradients keep adding up
        self._accumulated = 0
        if self.grad_clip > 0:               # (the global norm over the trained tables' gradients)
            grads = [t.grad for t in self.trained]
            self.engine.clip_grad_norm_(grads[0], grads[1] if len(grads) == 2 else None, self.grad_clip, self.grad_norm)
        self.optimizer_step(lazy_zero=self._last_full and self.accumulate == 1)
        self._grads_zero = True
        return loss


def _alias(index, field):
    return property(lambda self: getattr(self.tables[index], field), lambda self, value: setattr(self.tables[index], field, value))


# the per-letter names of the records' fields: step.sumE is step.ent.sum, step.dR = x sets step.rel.grad (callers, subclasses and
# tests know the step by these; its own methods go through the records)
for _index, _letter in enumerate("ER"):
    for _name, _field in (("", "param"), ("d", "grad"), ("sum", "sum"), ("m", "exp_avg"), ("v", "exp_avg_sq"),
                          ("adam_state", "adam_state"), ("rows", "row_steps")):
        setattr(FusedTrainStep, _name + _letter, _alias(_index, _field))


class GraphedTrainStep:
    """Replays one training step as a HIP graph (torch.cuda.CUDAGraph records the library's launches on the capture
    stream): a step is ~5 kernels of 5-80 us for the lookup models and ~50 for the token-pooled ones, so the Python /
    ctypes launch path, not the GPU, bounds small steps.  Shapes are fixed at capture: n_po, n_sp, the candidate
    count and a CAPACITY for the positives -- shorter lists are padded with (row -1, col INT32_MAX), which sort
    behind every candidate tile and are skipped by the kernels.  The dropout step counter lives on the device and is
    incremented inside the graph, so every replay draws new masks (okge_dropout.step_dev).

    `inner` is a FusedTrainStep or a TokenPooledTrainStep (anything with .step(batch), .device-resident state and a
    `step_dev` attribute)."""

    PAD_COL = 2 ** 31 - 1

    def __init__(self, inner, example: H.PrefixBatch, pos_capacity, normalizer=None, counter=None):
        refuse_single_device(inner, type(self).__name__)
        self.inner = inner
        dev = example.pos_row.device
        self.device = dev
        self.pos_capacity = int(pos_capacity)
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)      # noqa: E731
        self.static = H.PrefixBatch(
            po_rel=i32(example.n_po) if example.n_po else None, po_obj=i32(example.n_po) if example.n_po else None,
            sp_subj=i32(example.n_sp) if example.n_sp else None, sp_rel=i32(example.n_sp) if example.n_sp else None,
            pos_row=i32(self.pos_capacity), pos_col=i32(self.pos_capacity),
            cand_ids=None if example.cand_ids is None else i32(example.cand_ids.numel()),
            cand_first=example.cand_first, n_cand=example.n_cand, cand_unique=example.cand_unique)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev) if counter is None else counter
        inner.step_dev = self.counter
        self.normalizer = normalizer
        self._load(example)
        state = inner.state_tensors()
        saved, steps0 = [t.clone() for t in state], inner.steps
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # warm-up outside capture: workspaces get allocated
            for _ in range(2):
                inner.step(self.static, normalizer)
        torch.cuda.current_stream(dev).wait_stream(side)
        for t, s0 in zip(state, saved):                     # the warm-up steps must not count as training
            t.copy_(s0)
        inner.steps = steps0
        if counter is None:
            self.counter.fill_(steps0)
        del saved
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: a sharded step carries RCCL collectives, and the process group's watchdog thread polls the events of
        # earlier collectives while this thread captures -- under the default (global) mode that query aborts the process
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.counter += 1
            self.loss = inner.step(self.static, normalizer)

    def _load(self, b: H.PrefixBatch):
        s = self.static
        if b.n_po != s.n_po or b.n_sp != s.n_sp or b.n_candidates != s.n_candidates or b.nnz > self.pos_capacity:
            raise ValueError("batch shape differs from the captured one (n_po, n_sp, candidates fixed; positives <= capacity)")
        for name in ("po_rel", "po_obj", "sp_subj", "sp_rel", "cand_ids"):
            dst, src = getattr(s, name), getattr(b, name)
            if dst is not None:
                dst.copy_(src.reshape(-1), non_blocking=True)
        n = b.nnz
        s.pos_row[:n].copy_(b.pos_row, non_blocking=True)
        s.pos_col[:n].copy_(b.pos_col, non_blocking=True)
        if n < self.pos_capacity:
            s.pos_row[n:].fill_(-1)
            s.pos_col[n:].fill_(self.PAD_COL)

    def step(self, batch: H.PrefixBatch):
        """Copies the batch into the captured buffers and replays; returns the device loss (double[1])."""
        self._load(batch)
        return self.replay()

    def replay(self):
        """Replays on whatever the captured buffers hold (a producer may fill `self.static` directly)."""
        self.graph.replay()
        mark = getattr(self.inner, "mark_pending", None)      # (token-pooled step: deferred decay steps are owed again)
        if mark is not None:
            mark()
        return self.loss
