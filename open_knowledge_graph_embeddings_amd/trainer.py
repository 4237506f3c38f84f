"""Trainer-side surface of the hot path (openkge/trainer.py:32-113, :181-272; openkge/dataset.py:423-453).

``AddLossModule`` keeps the reference's constructor and ``forward`` signature and return triple
``(loss, hook_loss, all_outputs)``.  In training mode one fused HIP call computes the loss AND the gradients;
the returned loss is wired into autograd by a custom Function so the reference Trainer's
``(loss.sum() / normalizer).backward()`` (trainer.py:217-234) deposits them in ``weight.grad`` unchanged.
``compute_metrics`` mirrors OneToNMentionRelationDataset.compute_metrics on the HIP rank kernel.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
from torch.nn import BCEWithLogitsLoss, KLDivLoss

import os

from . import hotpath as H
from .metrics import MetricResult
from .model import LookupBaseRelationEmbedder
from .virtual_tables import VirtualTables

CALLER_THREAD_BACKWARD = os.environ.get("OKGE_BACKWARD_ON_CALLER_THREAD", "1") == "1"
FAST_CALL = os.environ.get("OKGE_DROPIN_FAST", "1") == "1"      # the lookup route refills persistent argument structs (off: a fresh set per call)


class _FusedLossFn(torch.autograd.Function):
    """Autograd node standing for AddLossModule's whole forward: the gradients were already produced by the fused kernel,
    multiplied by `applied` = the 1 / (B N) the reference Trainer divides the summed loss by (dataset.py:935, trainer.py:221).
    backward compares that with the upstream scalar autograd delivers -- on the device, no host read -- and rescales only
    if they differ (one launch that reads a single float when they agree; before: two passes over 11.6 MB)."""

    @staticmethod
    def forward(ctx, e_weight, r_weight, loss, g_e, g_r, engine, applied, row_ids):
        """row_ids: None (g_e / g_r are dense table gradients) or the occurrence ids (ids_e, ids_r) of gradient ROWS
        (AddLossModule(sparse_grads=True)): backward then hands autograd uncoalesced sparse tensors, as the backward of
        nn.Embedding(sparse=True) does (model.py:390-391).  g_e or g_r None: that table is frozen (requires_grad False), the
        call computed no gradient for it and backward returns None for that input"""
        ctx.g_e, ctx.g_r, ctx.engine, ctx.applied = g_e, g_r, engine, applied
        ctx.row_ids, ctx.shapes = row_ids, (e_weight.shape, r_weight.shape)
        return loss.to(torch.float32).reshape(())               # (the cast already yields a fresh tensor)

    @staticmethod
    def backward(ctx, grad_out):
        alpha = grad_out.reshape(1).to(torch.float32).contiguous()
        g_e, g_r, ctx.g_e, ctx.g_r = ctx.g_e, ctx.g_r, None, None   # no reference left behind: AccumulateGrad then TAKES the
        if g_e is None or g_r is None:                              # a frozen table: the trained one's gradient alone
            ctx.engine.rescale_gradients_(g_r if g_e is None else g_e, None, alpha, ctx.applied)
            return g_e, g_r, None, None, None, None, None, None
        ctx.engine.rescale_gradients_(g_e, g_r, alpha, ctx.applied) # buffers as .grad instead of copying them (an 11.6 MB
        if ctx.row_ids is not None:                                 # copy per step at FB15k-237)
            (ids_e, ids_r), ctx.row_ids = ctx.row_ids, None         # (the rescale above acted on the value rows)
            g_e = torch.sparse_coo_tensor(ids_e[None].long(), g_e, ctx.shapes[0])
            g_r = torch.sparse_coo_tensor(ids_r[None].long(), g_r, ctx.shapes[1])
        return g_e, g_r, None, None, None, None, None, None


class _FusedLossHookFn(torch.autograd.Function):
    """_FusedLossFn with the l2_reg hook as a second output (AddLossModule(fused_l2_reg=True)): the fused calls left the
    gradient of loss + hook, times `applied`, in g_e / g_r, so the reference Trainer's `(loss.sum() + hook) / normalizer`
    (trainer.py:217-221) hands both outputs the same upstream scalar; the loss's is the one compared with `applied`."""

    @staticmethod
    def forward(ctx, e_weight, r_weight, loss, reg, g_e, g_r, engine, applied, row_ids):
        ctx.g_e, ctx.g_r, ctx.engine, ctx.applied = g_e, g_r, engine, applied
        ctx.row_ids, ctx.shapes = row_ids, (e_weight.shape, r_weight.shape)
        return loss.to(torch.float32).reshape(()), reg.to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, grad_loss, grad_hook):
        return _FusedLossFn.backward(ctx, grad_loss) + (None,)


def _flat(t):
    return None if t is None else t.reshape(-1)


def _check_sorted(pos_col):
    """OKGE_VALIDATE: one host read"""
    if pos_col.numel() > 1 and bool((pos_col[1:] < pos_col[:-1]).any()):
        raise ValueError("coordinate labels must be sorted by column (the kernels partition them by candidate tile)")


def _ids(dev, *tensors):
    """the tensors (None stays None) as flat contiguous int32 tensors on dev -- themselves when their memory already is that (the
    kernels read a pointer and a count): one pass, no new tensor object on the common call"""
    for t in tensors:
        if t is not None and (t.dtype != torch.int32 or t.device != dev or not t.is_contiguous()):
            return [H._i32(x, dev) for x in tensors]
    return tensors


class _VirtualTablesLossFn(torch.autograd.Function):
    """Loss of already ENCODED rows (embedder variants that fall through to torch): the rows of one batch form the two small
    virtual tables EV / RV and `vb` names positions in them (virtual_tables.py defines the layout) -- the fused HIP
    step runs on them without dropout (it was applied by the encode) and returns the dense row gradients, which autograd
    carries back through the projection / batch-norm / normalisation into the parameters."""

    @staticmethod
    def forward(ctx, EV, RV, engine, scorer, vb, kind, smoothing, scores):
        EVc, RVc = EV.detach().contiguous(), RV.detach().contiguous()
        # every row of the two virtual tables is one candidate or one batch row: all of them are STORED by the call
        dEV, dRV = torch.empty_like(EVc), torch.empty_like(RVc)
        loss = engine.forward_backward(EVc, RVc, scorer, vb, dEV, dRV, loss=kind, label_smoothing=smoothing, normalizer=1.0,
                                       scores=scores, grads_zero=True, distinct_prefix_rows=True)
        ctx.engine, ctx.grads = engine, (dEV, dRV)
        return loss.to(torch.float32).reshape(())               # (the cast already yields a fresh tensor)

    @staticmethod
    def backward(ctx, grad_out):
        alpha = grad_out.reshape(1).to(torch.float32).contiguous()
        grads, ctx.grads = ctx.grads, None
        for g in grads:
            ctx.engine.scale_(g, alpha)
        return grads[0], grads[1], None, None, None, None, None, None


class _TokenPooledLossFn(torch.autograd.Function):
    """AddLossModule's forward for the token-pooled models: the fused step on the pooled rows + the pooling / batch-norm
    backward already left the dense gradients of the SUMMED loss in the slots; backward scales them by the upstream
    scalar and hands them to autograd in the order of `params`."""

    @staticmethod
    def forward(ctx, loss, engine, grads, *params):
        ctx.engine, ctx.grads = engine, grads
        return loss.to(torch.float32).reshape(()).clone()

    @staticmethod
    def backward(ctx, grad_out):
        alpha = grad_out.reshape(1).to(torch.float32).contiguous()
        for g in ctx.grads:
            ctx.engine.scale_(g, alpha)
        return (None, None, None) + tuple(ctx.grads)


class AddLossModule(nn.Module):
    """openkge/trainer.py:32-113.

    `training_outputs=False` (not in the reference's signature) skips materialising `all_outputs` in TRAINING mode and
    returns None in its place: the reference's Trainer reads the predictions only in evaluation (trainer.py:258-272), and
    the (B, N) block is the one thing the fused training kernels never need to write (29.8 MB per step at FB15k-237)."""

    def __init__(self, model, loss, bce_label_smoothing=0.0, training_outputs=True, sparse_grads=False, fused_l2_reg=False,
                 fused_variants=False):
        super().__init__()
        self.model = model
        self.loss = loss
        self.bce_label_smoothing = bce_label_smoothing
        self.training_outputs = training_outputs
        # sparse_grads (not in the reference's signature; what model_config.sparse selects there, model.py:390-391): in training
        # mode the two embedding weights receive UNCOALESCED sparse gradients -- one value row per candidate / prefix occurrence,
        # stored by the fused step -- for an optimizer with a sparse branch (OkgeAdagrad, weight_decay = 0)
        self.sparse_grads = bool(sparse_grads)
        # fused_l2_reg (not in the reference's signature; opt-in as sparse_grads is): a lookup ComplEx / DistMult model whose ONLY
        # _encode variant is l2_reg (model.py:471-479) takes the fused step instead of the torch fall-through; the hook's value
        # and gradient come from okge_n3_forward_backward, issued behind the step on the same buffers, and `hook_loss` is
        # returned attached to the graph.  With batch_shared_entities None the fused step draws ONE candidate mask for both
        # directions where the reference draws one per direction: the hook is then twice one term -- exact without dropout,
        # equal in expectation with it.
        self.fused_l2_reg = bool(fused_l2_reg)
        # fused_variants (not in the reference's signature; opt-in as sparse_grads and fused_l2_reg are): a lookup ComplEx /
        # DistMult model with batch_norm, project_entity, normalize='norm' or l2_reg on takes the HIP encode and its backward
        # (lookup_variants.LookupVariantTrainStep) for every batch that has ONE shared candidate block -- batch_shared_entities
        # given, or eval mode.  A training batch with batch_shared_entities None (one candidate block per direction) keeps the
        # torch fall-through below.
        self.fused_variants = bool(fused_variants)
        if self.fused_variants:
            if self.fused_l2_reg or self.sparse_grads:
                raise NotImplementedError("fused_variants=True goes with neither fused_l2_reg (l2_reg is part of it) nor sparse_grads "
                                          "(the HIP encode returns dense gradients)")
            if hasattr(model, "entity_token_ids") or getattr(model, "fused_step_model", False) \
                    or not getattr(model, "encode_in_torch", False) or getattr(model, "scorer_name", None) not in ("complex", "distmult"):
                raise NotImplementedError("fused_variants=True is built for the ComplEx / DistMult lookup models with batch_norm, "
                                          "project_entity, normalize='norm' or l2_reg on (a plain lookup model takes the fused step as it "
                                          "is; Tucker3 and the token models bring their own)")
            from . import lookup_variants as LV
            LV.refuse_unsupported(model)
            LV.activation_name(model)
        if self.fused_l2_reg and (hasattr(model, "entity_token_ids") or getattr(model, "fused_step_model", False)
                                  or not hasattr(model, "entity_embedding") or not hasattr(model, "l2_reg")
                                  or getattr(model, "scorer_name", None) not in ("complex", "distmult")
                                  or getattr(model, "batch_norm", False) or getattr(model, "project_entity", False)
                                  or getattr(model, "normalize", "")):
            raise NotImplementedError("fused_l2_reg=True is built for the ComplEx / DistMult lookup models with l2_reg as their only "
                                      "_encode variant (no batch-norm, projection or normalisation; Tucker3 regularises its "
                                      "projected rows, the token embedders have no such keyword)")
        if self.sparse_grads and (hasattr(model, "entity_token_ids") or getattr(model, "fused_step_model", False)
                                  or (getattr(model, "encode_in_torch", False) and not self.fused_l2_reg)
                                  or not hasattr(model, "entity_embedding")
                                  or getattr(model, "scorer_name", None) not in ("complex", "distmult")):
            raise NotImplementedError("sparse_grads=True is built for the ComplEx / DistMult lookup models without batch-norm, "
                                      "projection or normalisation (the encoded-row and token models return dense gradients)")
        if isinstance(loss, (BCEWithLogitsLoss, KLDivLoss)) and loss.reduction != "sum":
            # trainer.py:106 sums whatever the loss returns and scripts/train.py builds both losses with reduction='sum';
            # the fused kernels produce exactly that sum -- any other reduction would be silently different
            raise NotImplementedError(f"loss.reduction={loss.reduction!r}: the fused path implements reduction='sum' "
                                      f"(scripts/train.py:92-99)")

    def _in_torch(self, m):
        """the model's embedder falls through to torch for the encode (model.py): not on the fused_l2_reg route"""
        return getattr(m, "encode_in_torch", False) and not self.fused_l2_reg

    def _n3_term(self, m, n_po, n_sp, batch_shared_entities):
        """(coef, cand_passes) of the fused l2_reg hook, or None when the model adds none (model.py:471: training mode only)"""
        if not (self.fused_l2_reg and m.training and m.l2_reg > 0):
            return None
        passes = (int(n_po > 0) + int(n_sp > 0)) if batch_shared_entities is None else 1
        return H.n3_coef(m.l2_reg, m.dropout), passes

    def _loss_kind(self):
        if isinstance(self.loss, KLDivLoss):
            return "kl"
        if isinstance(self.loss, BCEWithLogitsLoss):
            return "bce"
        raise NotImplementedError(f"{self.loss} not supported. Please choose either BCEWithLogitsLoss or KLDivLoss")

    def _frozen_table(self, m, n3=None):
        """The reference's resume_freeze (trainer.py:532-536) as the fused call sees it: requires_grad of the two tables, read on
        every call.  -> None (both trained), "entities" / "relations" (that one is frozen: OKGE_TRAIN_FREEZE_*, no gradient
        buffer, backward returns None for it) or "both" (nothing to train: the loss-only route).
        With sparse_grads=True or the fused l2_reg hook (n3) one frozen table also answers None: the occurrence-row call and the
        N3 kernel are not built for a missing buffer, so the whole step runs as it always did and autograd drops the gradient of
        the input that does not require one -- the frozen parameter's .grad stays None either way"""
        ge, gr = m.entity_embedding.weight.requires_grad, m.relation_embedding.weight.requires_grad
        if ge and gr:
            return None
        if not ge and not gr:
            return "both"
        if self.sparse_grads or n3 is not None:
            return None
        return "relations" if ge else "entities"

    @staticmethod
    def _candidates(m, use_batch_shared_entities, batch_shared_entities):
        """-> (cand_ids or None, first_id, n): all entities [min_entities_size, entities_size) without batch_shared_entities and in
        eval without batch sharing (trainer.py:77-78), else the shared id list -- which IS that range when it has its length and
        batch sharing is off: arange(vocab)[offset:] (dataset.py:872)"""
        n_ent, first = m.train_data.entities_size, m.train_data.min_entities_size
        if batch_shared_entities is None or (not use_batch_shared_entities and not m.training):
            return None, first, n_ent - first
        n = batch_shared_entities.numel()
        if n == n_ent - first and not use_batch_shared_entities:
            return None, first, n
        return batch_shared_entities, first, n

    @staticmethod
    def _wants_grad(m):
        want_grad = torch.is_grad_enabled() and m.training
        if want_grad and CALLER_THREAD_BACKWARD and torch.autograd.is_multithreading_enabled():
            # The caller's `loss.backward()` (trainer.py:226) hands a CUDA graph to the autograd engine's device thread and waits
            # for it: ~35 us of thread hand-off per step on a graph of ONE node whose backward only returns the gradients this
            # forward already computed (0.199 -> 0.162 ms per drop-in step, S-FB).  Run it on the calling thread instead
            # (thread-local autograd state; it stays set for this thread).  OKGE_BACKWARD_ON_CALLER_THREAD=0 leaves autograd alone.
            torch.autograd.set_multithreading_enabled(False)
        return want_grad

    def _outputs(self, m, B, n, dev):
        """the (B, n) block of predictions, rows padded to a multiple of four floats; None where training does without it"""
        if self.training_outputs or not m.training:
            return torch.empty((B, (n + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :n]
        return None

    def forward(self, inputs, labels, use_batch_shared_entities, batch_shared_entities, epoch=-1,
                input_style_triple_or_prefix="triple"):
        allowed = ["triple", "right_and_left_prefix"]
        if input_style_triple_or_prefix not in allowed:
            raise Exception("input_style_triple_or_prefix not in {}".format(allowed))
        if input_style_triple_or_prefix != "right_and_left_prefix":
            return None                                            # trainer.py:64 has no else branch
        kind = self._loss_kind()
        m = self.model
        dev = m.entity_embedding.weight.device
        # (models that bring their own fused step -- autograd_step / loss_only: the token encoders, Tucker3 -- share one route)
        token_model = hasattr(m, "entity_token_ids") or getattr(m, "fused_step_model", False)
        if not token_model and not self._in_torch(m):
            return self._lookup_result(m, dev, kind, inputs, labels, use_batch_shared_entities, batch_shared_entities, epoch)
        po, sp = inputs
        batch = H.PrefixBatch()
        if po is not None:
            batch.po_rel, batch.po_obj = _flat(po[0]), _flat(po[1])
        if sp is not None:
            batch.sp_subj, batch.sp_rel = _flat(sp[0]), _flat(sp[1])
        batch.cand_ids, batch.cand_first, batch.n_cand = self._candidates(m, use_batch_shared_entities, batch_shared_entities)
        batch.cand_ids = _flat(batch.cand_ids)
        if isinstance(labels, tuple):                               # (pos_row, pos_col) coordinates, sorted by column
            if H.VALIDATE:
                _check_sorted(labels[1])
            batch.pos_row, batch.pos_col = labels
        else:                                                       # dense (B, N) {0,1} (dataset.py:885-932)
            batch.pos_row, batch.pos_col = H.positives_from_dense(labels.to(dev))
        want_grad = self._wants_grad(m)
        all_outputs = self._outputs(m, batch.B, batch.n_cand, dev)
        smoothing = self.bce_label_smoothing if kind == "bce" else 0.0
        if self.fused_variants and (not m.training or (want_grad and batch_shared_entities is not None)):
            # (the hook's gradient is part of the gradients the step leaves; its value is the step's, model.py:447-453)
            return self._own_step_result(m, batch, kind, smoothing, want_grad, all_outputs, None, step_hook=True)
        if self._in_torch(m):
            return self._variant_result(m, batch, kind, smoothing, want_grad, all_outputs, epoch,
                                        all_entities=not use_batch_shared_entities and not m.training,
                                        per_direction=batch_shared_entities is None)
        hook_loss = m.after_batch_loss_hook(epoch) if hasattr(m, "after_batch_loss_hook") else None
        return self._own_step_result(m, batch, kind, smoothing, want_grad, all_outputs, hook_loss)

    def _lookup_result(self, m, dev, kind, inputs, labels, use_batch_shared_entities, batch_shared_entities, epoch):
        """The plain lookup models: the call the reference Trainer makes thousands of times per epoch, and its loss-only form
        (eval mode, no_grad, both tables frozen).  The inputs become flat int32 device tensors -- the Trainer's already are, and
        are taken as they are -- and fill the four argument structs of a hotpath.PrefixCall, from which the step and, behind it
        on the same structs, the l2_reg hook are issued.  FAST_CALL: the structs are the module's own (`_fd`), refilled in place
        -- a fresh set per call is ~10 us of Python on a step whose kernels take 130 us (the path is host-bound, INTEGRATION.md
        section 1); under OKGE_VALIDATE they are fresh, and the ids are range-checked on the host first."""
        po, sp = inputs
        po_rel, po_obj = (None, None) if po is None else po
        sp_subj, sp_rel = (None, None) if sp is None else sp
        if isinstance(labels, tuple):                               # (pos_row, pos_col) coordinates, sorted by column
            if H.VALIDATE:
                _check_sorted(labels[1])
            pos_row, pos_col = labels
        else:                                                       # dense (B, N) {0,1} (dataset.py:885-932)
            pos_row, pos_col = H.positives_from_dense(labels.to(dev))
        cand, first, n = self._candidates(m, use_batch_shared_entities, batch_shared_entities)
        po_rel, po_obj, sp_subj, sp_rel, pos_row, pos_col, cand = _ids(dev, po_rel, po_obj, sp_subj, sp_rel, pos_row, pos_col, cand)
        want_grad = self._wants_grad(m)
        hook_loss = m.after_batch_loss_hook(epoch) if hasattr(m, "after_batch_loss_hook") else None
        if m.training:
            m.dropout_step += 1
        E, R, eng = m.E, m.R, m.engine()
        if H.VALIDATE:
            H.validate_ids(H.PrefixBatch(po_rel, po_obj, sp_subj, sp_rel, pos_row, pos_col, cand, first, n), E.shape[0], R.shape[0])
            call = H.PrefixCall()
        elif FAST_CALL:
            call = getattr(self, "_fd", None)
            if call is None:
                call = self._fd = H.PrefixCall()
        else:
            call = H.PrefixCall()
        call.fill_tables(E, R, m.scorer_name, eng.device)
        call.fill_ids(po_rel, po_obj, sp_subj, sp_rel, cand, first, n, pos_row, pos_col)
        if getattr(m.dropout_spec, "__func__", None) is LookupBaseRelationEmbedder.dropout_spec:
            # (the five DropoutSpec objects m.dropout_spec would build, written in place: same numbers)
            call.fill_dropout(m.keep_prob_dropout(m.input_dropout, m.dropout), m.keep_prob_dropout(m.relation_input_dropout, m.relation_dropout),
                              m.dropout_seed, m.dropout_step)
        else:                                                       # a model that answers dropout_spec itself (replayed `keep` masks)
            call.fill_dropout_specs([m.dropout_spec(stream, stream in (H.STREAM_PO_REL, H.STREAM_SP_REL)) for stream in H.STREAMS])
        B = call.B
        all_outputs = self._outputs(m, B, n, dev)
        smoothing = self.bce_label_smoothing if kind == "bce" else 0.0
        n3 = self._n3_term(m, call.n_po, call.n_sp, batch_shared_entities)
        frozen = self._frozen_table(m, n3) if want_grad else None
        # (fresh per call: autograd holds on to them)
        loss_out = torch.empty(1, dtype=torch.float64, device=dev)
        reg_out = torch.empty(1, dtype=torch.float64, device=dev) if n3 is not None else None
        if not want_grad or frozen == "both":                       # nothing to train: the loss, and the hook's value
            flags = H.train_flags(loss_only=True)
            result = call.train(eng, kind, smoothing, 1.0, flags, loss_out, None, None, all_outputs).to(torch.float32).reshape(())
            if n3 is not None:
                hook_loss = call.n3(eng, n3[0], n3[1], 1.0, flags, reg_out, None, None).to(torch.float32).reshape(())
            return result, hook_loss, all_outputs
        # a contiguous candidate range: the call stores the candidate rows and clears the rest itself (all of dR, the
        # reserved rows in front of the candidates) inside its first launch -- fresh buffers, no fill launches.
        # An id list: candidate rows accumulate, so the buffers start from zero.
        clear = cand is None and not self.sparse_grads
        row_ids = None
        if self.sparse_grads:                                       # occurrence rows, every one stored by the call
            g_e, g_r = E.new_empty((n + B, E.shape[1])), R.new_empty((B, R.shape[1]))
            row_ids = H.occurrence_ids(dev, cand, first, n, po_obj, sp_subj, po_rel, sp_rel)
        else:
            g_e, g_r = (torch.empty_like(E), torch.empty_like(R)) if clear else (torch.zeros_like(E), torch.zeros_like(R))
        if frozen is not None:                                      # the frozen table gets no buffer at all
            g_e, g_r = (None, g_r) if frozen == "entities" else (g_e, None)
        flags = H.train_flags(grads_zero=not self.sparse_grads, clear_grads=clear, row_grads=self.sparse_grads, freeze=frozen)
        # the factor the Trainer will apply (trainer.py:221: loss / normalizer_loss, normalizer_loss = B x N,
        # dataset.py:935) goes into the fused step; _FusedLossFn.backward checks it against what autograd delivers
        # (torch divides a fp32 tensor by a Python number as a multiplication by fp32(1) / fp32(number), forward and
        #  backward: `applied` is built the same way, and the normalizer handed to the library is the one whose fp32
        #  reciprocal is exactly that)
        applied = np.float32(1.0) / np.float32(float(B) * float(n))
        loss = call.train(eng, kind, smoothing, 1.0 / float(applied), flags, loss_out, g_e, g_r, all_outputs)
        weights = m.entity_embedding.weight, m.relation_embedding.weight
        if n3 is None:
            return _FusedLossFn.apply(*weights, loss, g_e, g_r, eng, float(applied), row_ids), hook_loss, all_outputs
        reg = call.n3(eng, n3[0], n3[1], 1.0 / float(applied), H.train_flags(row_grads=self.sparse_grads), reg_out, g_e, g_r)
        result, hook_loss = _FusedLossHookFn.apply(*weights, loss, reg, g_e, g_r, eng, float(applied), row_ids)
        return result, hook_loss, all_outputs

    def _variant_result(self, m, batch, kind, smoothing, want_grad, all_outputs, epoch, all_entities, per_direction):
        """lookup embedder with batch_norm / projection / normalize / l2_reg on (model.py:463-479): torch encodes in the
        reference's call order and the HIP scorer / loss / backward works on the encoded rows.
        With a shared id list (trainer.py:75-84): candidates once -- get_all_obj() in eval without batch sharing, else
        precompute_batch_shared_inputs -- then (rel, obj) of the po rows, (subj, rel) of the sp rows (model.py:52-74).
        With batch_shared_entities=None (trainer.py:86-87) each prefix scorer encodes its OWN candidate block:
        po_prefix_score get_all_subj() first, sp_prefix_score get_all_obj() last (model.py:60-61, :71-72) -- two blocks
        that differ under project_entity (subj_ vs obj_projection), and two batch-norm / l2-hook passes either way; the
        two directions then run as two fused calls whose losses add (reduction='sum' is a plain sum over rows)."""
        dev = m.entity_embedding.weight.device
        n_po, n_sp, n_c = batch.n_po, batch.n_sp, batch.n_candidates
        vt = VirtualTables(dev)                                                     # (one arange for the call's position batches)
        calls = []                                                                  # (EV, RV, virtual batch, output rows)
        with torch.set_grad_enabled(want_grad):
            if per_direction:
                # the positives of one direction WITHOUT a host synchronisation (boolean-mask indexing reads the count back):
                # the other direction's entries become padding -- (row -1, column INT32_MAX), which the kernels skip and which
                # sorts behind every candidate tile (okge.h, okge_positives) -- and a stable device sort restores column order
                pad_col = torch.iinfo(torch.int32).max

                def direction_positives(keep, row_shift):
                    col = torch.where(keep, batch.pos_col, torch.full_like(batch.pos_col, pad_col))
                    row = torch.where(keep, batch.pos_row - row_shift, torch.full_like(batch.pos_row, -1))
                    order = torch.argsort(col, stable=True)
                    return row[order].contiguous(), col[order].contiguous()
                in_po = batch.pos_row < n_po
                if n_po:
                    cand = m.get_all_subj().reshape(n_c, -1)
                    rel = m.encode_rel(batch.po_rel).reshape(n_po, -1)
                    obj = m.encode_obj(batch.po_obj).reshape(n_po, -1)
                    prow, pcol = direction_positives(in_po, 0)
                    vb = vt.batch(n_c, n_po, 0, prow, pcol)
                    calls.append((torch.cat([cand, obj]), rel, vb, slice(0, n_po)))
                if n_sp:
                    subj = m.encode_subj(batch.sp_subj).reshape(n_sp, -1)
                    rel = m.encode_rel(batch.sp_rel).reshape(n_sp, -1)
                    cand = m.get_all_obj().reshape(n_c, -1)
                    prow, pcol = direction_positives(~in_po, n_po)
                    vb = vt.batch(n_c, 0, n_sp, prow, pcol)
                    calls.append((torch.cat([cand, subj]), rel, vb, slice(n_po, n_po + n_sp)))
            else:
                if all_entities:
                    cand = m.get_all_obj()
                elif batch.cand_ids is not None:
                    cand = m.precompute_batch_shared_inputs(batch.cand_ids)
                else:
                    cand = m.precompute_batch_shared_inputs(torch.arange(batch.cand_first, batch.cand_first + n_c, dtype=torch.int32,
                                                                         device=dev))
                parts_e, parts_r = [cand.reshape(n_c, -1)], []
                if n_po:
                    parts_r.append(m.encode_rel(batch.po_rel).reshape(n_po, -1))
                    parts_e.append(m.encode_obj(batch.po_obj).reshape(n_po, -1))
                if n_sp:
                    parts_e.append(m.encode_subj(batch.sp_subj).reshape(n_sp, -1))
                    parts_r.append(m.encode_rel(batch.sp_rel).reshape(n_sp, -1))
                vb = vt.batch(n_c, n_po, n_sp, batch.pos_row, batch.pos_col)
                calls.append((torch.cat(parts_e), torch.cat(parts_r), vb, slice(0, n_po + n_sp)))
        hook_loss = m.after_batch_loss_hook(epoch)
        eng = m.engine()
        result = None
        for EV, RV, vb, rows in calls:
            out = all_outputs[rows] if all_outputs is not None else None
            if want_grad:
                part = _VirtualTablesLossFn.apply(EV, RV, eng, m.scorer_name, vb, kind, smoothing, out)
            else:
                part = eng.forward_backward(EV.detach().contiguous(), RV.detach().contiguous(), m.scorer_name, vb, None, None,
                                            loss=kind, label_smoothing=smoothing, normalizer=1.0, scores=out,
                                            loss_only=True).to(torch.float32).reshape(())
            result = part if result is None else result + part
        return result, hook_loss, all_outputs

    def _own_step_result(self, m, batch, kind, smoothing, want_grad, all_outputs, hook_loss, step_hook=False):
        """Models that bring their own step (autograd_step / autograd_params_and_grads / loss_only).  The UnigramPooling* models
        (model.py:716-796) and Tucker3: the encoded rows of the batch form two small virtual tables, the fused step runs on them,
        and the encoder's backward deposits dense parameter gradients.  AddLossModule(fused_variants=True), step_hook: the lookup
        embedder's variants on the HIP encode through the same protocol; the step's normalizer is 1 and the hook's gradient is
        part of the gradients it leaves, so `(loss.sum() + hook) / normalizer` (trainer.py:217-221) scales both by the upstream
        scalar of the loss, and the hook's value is the step's (model.py:447-453: training mode, l2_reg > 0)."""
        if not want_grad:
            return m.loss_only(batch, kind, smoothing, all_outputs).to(torch.float32).reshape(()), hook_loss, all_outputs
        st = m.autograd_step(kind, smoothing)
        loss = st.forward_backward(batch, normalizer=1.0, scores=all_outputs)
        params, grads = m.autograd_params_and_grads(st)
        result = _TokenPooledLossFn.apply(loss, m.engine(), grads, *params)
        if step_hook and m.l2_reg > 0:
            hook_loss = st.reg_out.to(torch.float32).reshape(())
        return result, hook_loss, all_outputs


def compute_metrics(filter_mask, label_ids, predictions, engine: H.HotPath = None) -> MetricResult:
    """OneToNMentionRelationDataset.compute_metrics (dataset.py:423-453) on the HIP rank kernel.

    filter_mask (B, N) bool; label_ids list[B] of list[G_b] of int tensors (candidate-relative ids);
    predictions (B, N) fp32 on the GPU.  Returns the same seven meters, weighted by number of groups per row."""
    dev = predictions.device
    engine = engine or H.HotPath(dev)
    row_ptr, grp_ptr, ids = [0], [0], []
    for groups in label_ids:
        for g in groups:
            ids.extend(int(x) for x in g.reshape(-1).tolist())
            grp_ptr.append(len(ids))
        row_ptr.append(len(grp_ptr) - 1)
    fm = filter_mask.to(dev)
    nz = fm.nonzero()                                            # sorted by row: CSR columns
    filt_ptr = torch.zeros(fm.shape[0] + 1, dtype=torch.int64, device=dev)
    filt_ptr[1:] = torch.cumsum(fm.sum(1), 0)
    filt_col = nz[:, 1].to(torch.int32).contiguous()
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)        # noqa: E731
    preds = predictions if predictions.stride(1) == 1 else predictions.contiguous()
    ranks = engine.filtered_ranks(preds, filt_ptr, filt_col, t(row_ptr, torch.int64), t(grp_ptr, torch.int64),
                                  t(ids, torch.int32)).cpu()
    result = MetricResult()
    for b in range(len(label_ids)):
        r = ranks[row_ptr[b]:row_ptr[b + 1]]
        n = int(r.numel())
        if n == 0:
            continue
        result["mrr"].update((1.0 / (r + 1).float()).sum().item() / n, n)
        result["mr"].update(r.sum().item() / n, n)
        for k in (50, 10, 3, 1):
            result[f"h{k}"].update((r < k).float().sum().item() / n, n)
    return result
