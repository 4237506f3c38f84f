"""LSTM-encoded embedder: LSTMRelationEmbedder + LSTM{Complex,Distmult}RelationModel (openkge/model.py:912-998, :1026-1034)
over the HIP kernels of csrc/okge_lstm.hip (forward and backward through time on the exact-fp32 MFMA), and the training
step that drives the fused prefix-scoring path on rows encoded from tokens.

The step is virtual_tables.VirtualTableStep (layout and skeleton, shared with token_pooled.py) with the LSTM as the encoder:
the fused step's dense row gradients go back through batch-norm and the LSTM into the token tables, the LSTM weights and the
batch-norm parameters.  The three entity calls share one LSTM pass and the two relation calls another; batch-norm statistics
stay per call, in the reference's order (trainer.py:75-91).  The dense Adagrad then moves every parameter, as the reference's
optimizer does.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N
from . import hotpath as H
from .model import ComplexRelationScorer, DistmultRelationScorer, Models
from . import virtual_tables as VT
from .token_pooled import BN_EPS, BN_MOMENTUM, UnigramPoolingRelationEmbedder, token_id_matrix

MAX_SLOT = 512                                     # the fused tile kernels' largest slot size
PRECOMPUTE_CHUNK = 16384                           # rows per encode call of precompute_embeddings_from_tokens


class LSTMSlot:
    """One embedder slot (entity or relation): token table, token-id matrix, the four nn.LSTM tensors, optional batch-norm,
    gradients and Adagrad accumulators."""

    def __init__(self, W, token_ids, lstm, bn=None, running=None, flat=None):
        """lstm: [weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0]; bn: [weight, bias] or None; running: (mean, var);
        flat: one buffer the four LSTM tensors are views of (one optimizer segment instead of four), or None"""
        self.W, self.token_ids = W, token_ids.to(torch.int32).contiguous()
        self.d, self.L = W.shape[1], self.token_ids.shape[1]
        self.lstm, self.flat = list(lstm), flat
        dev = W.device
        self.dW = torch.zeros_like(W)
        self.sumW = torch.zeros_like(W)
        self.fresh_lstm_grads()
        self.sum_flat = torch.zeros_like(self.d_flat)
        self.bn = None
        if bn is not None:
            d = self.d
            self.bn = torch.cat([bn[0].reshape(-1), bn[1].reshape(-1)]).to(device=dev, dtype=torch.float32).contiguous()
            self.running_mean, self.running_var = running
            self.d_bn = torch.zeros(2 * d, dtype=torch.float32, device=dev)
            self.sum_bn = torch.zeros(2 * d, dtype=torch.float32, device=dev)

    def fresh_lstm_grads(self):
        """d_flat: one zeroed gradient buffer; dlstm: the four LSTM tensors' gradients as views of it"""
        self.d_flat = torch.zeros(sum(p.numel() for p in self.lstm), dtype=torch.float32, device=self.W.device)
        self.dlstm = [g.view_as(p) for g, p in zip(self.d_flat.split([p.numel() for p in self.lstm]), self.lstm)]

    def c(self):
        s = N.LstmSlot()
        s.W, s.token_ids = self.W.data_ptr(), self.token_ids.data_ptr()
        s.vocab, s.d, s.n_ids, s.max_len = self.W.shape[0], self.d, self.token_ids.shape[0], self.L
        s.w_ih, s.w_hh, s.b_ih, s.b_hh = (p.data_ptr() for p in self.lstm)
        if self.bn is not None:
            s.bn_weight, s.bn_bias = self.bn[:self.d].data_ptr(), self.bn[self.d:].data_ptr()
            s.bn_running_mean, s.bn_running_var = self.running_mean.data_ptr(), self.running_var.data_ptr()
            s.bn_eps, s.bn_momentum = BN_EPS, BN_MOMENTUM
        return s

    def optimizer_tensors(self):
        if self.flat is None:
            raise RuntimeError("the slot's own optimizer needs its LSTM tensors in one flat buffer")
        out = [(self.W, self.dW, self.sumW), (self.flat, self.d_flat, self.sum_flat)]
        if self.bn is not None:
            out.append((self.bn, self.d_bn, self.sum_bn))
        return out


class LstmPass:
    """The workspace of one LSTM pass (a slot's calls of one step) and its ctypes driver (okge_lstm_encode_calls /
    okge_lstm_backward_calls).  A backward needs the workspace its forward left: one object per pass in flight."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.lib = N.lib()
        self.ws, self.ws_bytes = None, 0
        self.pos_tok = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _calls(self, calls):
        arr = (N.LstmCall * len(calls))()
        for x, (ids, first_id, n) in zip(arr, calls):
            x.ids, x.first_id, x.n = None if ids is None else ids.data_ptr(), int(first_id), int(n)
        return arr

    def encode(self, slot: LSTMSlot, calls, training, raw, out):
        """calls: [(ids int32 or None, first_id, n)] with n > 0, their rows one after the other in raw / out ([rows][ld])"""
        rows = sum(int(c[2]) for c in calls)
        need = int(self.lib.okge_lstm_workspace_bytes(rows, slot.L, slot.d, int(bool(training))))
        if need > self.ws_bytes:
            self.ws, self.ws_bytes = torch.empty(need, dtype=torch.uint8, device=self.device), need
        if self.pos_tok is None or self.pos_tok.numel() < rows * slot.L:
            self.pos_tok = torch.empty(rows * slot.L, dtype=torch.int32, device=self.device)
        self.rows, self.trained = rows, bool(training)
        s = slot.c()
        N.check(self.lib.okge_lstm_encode_calls(ctypes.byref(s), self._calls(calls), len(calls), int(bool(training)), raw.data_ptr(),
                                                out.data_ptr(), raw.stride(0), self.pos_tok.data_ptr(), self.ws.data_ptr(),
                                                self.ws_bytes, self._stream()), "okge_lstm_encode_calls")

    def backward(self, slot: LSTMSlot, calls, raw, d_out, dW, dlstm, d_bn):
        """after encode(slot, calls, training=True, raw, ...): dW += token-row gradients; dlstm (4 tensors), d_bn ([w | b])
        are written"""
        if not self.trained:
            raise RuntimeError("LSTM backward without a training-mode forward")
        pos = self.pos_tok[:self.rows * slot.L]
        order = torch.argsort(pos, stable=True).to(torch.int32)           # (index plumbing; the sums are the kernel's)
        s = slot.c()
        d = slot.d
        bn = slot.bn is not None
        N.check(self.lib.okge_lstm_backward_calls(ctypes.byref(s), self._calls(calls), len(calls), raw.data_ptr(), d_out.data_ptr(),
                                                  raw.stride(0), pos.data_ptr(), order.data_ptr(), dW.data_ptr(),
                                                  *(g.data_ptr() for g in dlstm), d_bn[:d].data_ptr() if bn else None,
                                                  d_bn[d:].data_ptr() if bn else None, self.ws.data_ptr(), self.ws_bytes,
                                                  self._stream()), "okge_lstm_backward_calls")


class LSTMTrainStep(VT.VirtualTableStep):
    """forward + loss + backward + Adagrad for LSTM{Complex,Distmult}RelationModel (Trainer.compute_one_batch,
    trainer.py:181-257, over model.py:966-998).  The optimizer is dense: every token row, LSTM tensor and batch-norm parameter
    moves every step (utils/optim.py:139-160).

    With the "bias_entity" scorer (DataBiasOnlyEntityModel, model.py:317-350, :1036-1039) the relation slot never reaches the
    score: the reference's backward leaves every relation parameter without a gradient and torch's Adagrad skips them.  Here
    the relation slot is then encoded forward only, and only behind a batch-norm (its running statistics still move: the
    encode runs in training mode, model.py:58-59, :72-73); no backward through it, and optimizer_step() touches neither its
    parameters nor its gradients nor its accumulators.  "bias_relation" is the ordinary step: the prefix entities' gradient
    rows arrive as zeros."""

    bias_scorers = True

    def __init__(self, entity: LSTMSlot, relation: LSTMSlot, scorer, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8,
                 label_smoothing=0.0, dropout=0.0, relation_dropout=None, seed=0, engine=None):
        super().__init__(entity, relation, scorer, loss=loss, lr=lr, weight_decay=weight_decay, eps=eps,
                         label_smoothing=label_smoothing, dropout=dropout, relation_dropout=relation_dropout, seed=seed, engine=engine)
        self.passes = (LstmPass(self.device), LstmPass(self.device))
        self.decay_window = 1
        self.relation_unused = scorer == "bias_entity"

    def state_tensors(self):
        out = []
        for sl in (self.entity, self.relation):
            out += [sl.W, sl.dW, sl.sumW, sl.flat, sl.d_flat, sl.sum_flat]
            if sl.bn is not None:
                out += [sl.bn, sl.d_bn, sl.sum_bn, sl.running_mean, sl.running_var]
        return out

    def flush(self):
        """(no deferred updates here: every parameter is current after every step)"""

    def _encode(self, batch: H.PrefixBatch, bufs):
        """one LSTM pass per slot over its calls, in the reference's encode order; -> the two slots' non-empty calls"""
        dev = self.device
        EV, EX, dEV, RV, RX, dRV = bufs
        calls = ([], [])
        for relation, ids, first, rows in VT.encode_calls(batch):
            if rows.stop > rows.start:
                calls[relation].append((H._i32(ids, dev), first, rows.stop - rows.start))
        self.passes[0].encode(self.entity, calls[0], True, EX, EV)
        if not self.relation_unused or self.relation.bn is not None:      # (unused: only for the running statistics)
            self.passes[1].encode(self.relation, calls[1], True, RX, RV)
        return calls

    def _backward(self, batch, bufs, calls):
        """dEV / dRV -> batch-norm and the LSTM backward through time -> the slots' dW, d_flat (dlstm), d_bn ([d weight | d bias])"""
        EV, EX, dEV, RV, RX, dRV = bufs
        for ps, sl, cs, X, dV in zip(self.passes, (self.entity, self.relation), calls, (EX, RX), (dEV, dRV)):
            if sl is self.relation and self.relation_unused:
                continue
            ps.backward(sl, cs, X, dV, sl.dW, sl.dlstm, sl.d_bn if sl.bn is not None else None)

    def optimizer_step(self):
        tensors = self.entity.optimizer_tensors() + ([] if self.relation_unused else self.relation.optimizer_tensors())
        for i in range(0, len(tensors), 4):                       # (okge_adagrad_multi: up to four tensors per launch)
            self.engine.adagrad_multi(tensors[i:i + 4], self.lr, self.weight_decay, self.eps)
        self._sync_module_batchnorms()


class LSTMEncodeFn(torch.autograd.Function):
    """encode_* with gradients enabled (a caller's own loss): the HIP forward and backward through time of ONE call, with a
    workspace of its own (kept until backward).  Inputs after the first three are the slot's parameters, so that autograd
    hands their gradients on: W, weight_ih, weight_hh, bias_ih, bias_hh[, bn weight, bn bias]."""

    @staticmethod
    def forward(ctx, ids, module, relation, W, w_ih, w_hh, b_ih, b_hh, *bn):
        slot = module._slot(relation, detach=True)
        n, d = ids.numel(), slot.d
        raw = torch.empty((n, d), device=ids.device)
        out = torch.empty_like(raw) if slot.bn is not None else raw
        ps = LstmPass(ids.device)
        training = module.training
        ps.encode(slot, [(ids, 0, n)], training, raw, out)
        ctx.slot, ctx.ps, ctx.ids, ctx.raw, ctx.training = slot, ps, ids, raw, training
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.training:
            raise RuntimeError("gradients of an eval-mode LSTM encode are not implemented (the running statistics have no graph)")
        slot = ctx.slot
        d = slot.d
        dW = torch.zeros_like(slot.W)
        dl = [torch.empty_like(p) for p in slot.lstm]
        d_bn = torch.empty(2 * d, device=g.device) if slot.bn is not None else None
        ctx.ps.backward(slot, [(ctx.ids, 0, ctx.ids.numel())], ctx.raw, g.contiguous(), dW, dl, d_bn)
        bn_grads = () if d_bn is None else (d_bn[:d].clone(), d_bn[d:].clone())
        return (None, None, None, dW, *dl, *bn_grads)


# ------------------------------------------------------------------------------------------------------------------
# API-compatible model classes
# ------------------------------------------------------------------------------------------------------------------
class LSTMRelationEmbedder(UnigramPoolingRelationEmbedder):
    """openkge/model.py:912-998.  Implemented: normalize None|''|'batchnorm', dropout / entity_dropout / relation_dropout
    (Philox masks), slot sizes up to 512; not implemented (raise at construction): encoder_activiation, project_relation,
    sparse, relation_slot_size != entity_slot_size.  Training: LSTMTrainStep (fused, own dense Adagrad) or
    trainer.AddLossModule (autograd bridge: any torch optimizer over the module's parameters).  The evaluation surface
    (precompute_embeddings_from_tokens, get_all_* / get_*, prefix scores, loss_only) is the token-pooled embedder's."""

    def __init__(self, entity_slot_size, relation_slot_size, train_data, dropout=0.0, entity_dropout=None, relation_dropout=None,
                 encoder_activiation=None, sparse=False, init_std=0.1, normalize='', project_relation=False, seed=0):
        torch.nn.Module.__init__(self)
        if relation_slot_size is None or relation_slot_size <= 0:
            relation_slot_size = entity_slot_size
        if encoder_activiation is not None:
            raise NotImplementedError("encoder_activiation: the reference applies a module class to a tensor (model.py:976-977)")
        if project_relation:
            raise NotImplementedError("project_relation is not implemented for the LSTM embedder")
        if sparse:
            raise NotImplementedError("sparse gradients are not implemented for the LSTM embedder")
        if relation_slot_size != entity_slot_size:
            raise NotImplementedError("relation slot size must equal the entity slot size")
        if entity_slot_size > MAX_SLOT:
            raise NotImplementedError(f"LSTM slot sizes above {MAX_SLOT}")
        if normalize not in (None, '', 'batchnorm'):
            raise NotImplementedError(f"normalize={normalize!r}")
        self.train_data, self.slot_size, self.relation_slot_size = train_data, entity_slot_size, relation_slot_size
        self.normalize = normalize
        # the reference's constructor order (TokenBasedRelationEmbedder.__init__, model.py:568-631, then :932-952): the same
        # torch.manual_seed gives bit-identical initial parameters
        max_len = train_data.max_length
        e_len, r_len = (max_len, max_len) if isinstance(max_len, int) else (max_len[0], max_len[1])
        self.register_buffer('entity_token_ids', token_id_matrix(train_data.entity_id_to_tokens_map, e_len))
        self.register_buffer('relation_token_ids', token_id_matrix(train_data.relation_id_to_tokens_map, r_len))
        self.entity_embedding = torch.nn.Embedding(train_data.entity_tokens_size, entity_slot_size, padding_idx=0)
        self.relation_embedding = torch.nn.Embedding(train_data.relation_tokens_size, relation_slot_size, padding_idx=0)
        self.entity_batchnorm = self.relation_batchnorm = None
        if normalize == 'batchnorm':
            self.entity_batchnorm = torch.nn.BatchNorm1d(entity_slot_size, momentum=BN_MOMENTUM, eps=BN_EPS)
            self.relation_batchnorm = torch.nn.BatchNorm1d(relation_slot_size, momentum=BN_MOMENTUM, eps=BN_EPS)
            torch.nn.init.uniform_(self.entity_batchnorm.weight)
            torch.nn.init.uniform_(self.relation_batchnorm.weight)
        torch.nn.init.normal_(self.entity_embedding.weight.data, std=init_std)          # row 0 included
        torch.nn.init.normal_(self.relation_embedding.weight.data, std=init_std)
        # (nn.LSTM warns that dropout has no effect on one layer; kept as the reference passes it)
        self.entity_encoder_in = torch.nn.LSTM(input_size=entity_slot_size, hidden_size=entity_slot_size, batch_first=True, dropout=dropout)
        self.relation_encoder_in = torch.nn.LSTM(input_size=relation_slot_size, hidden_size=relation_slot_size, batch_first=True,
                                                 dropout=dropout)
        self.entity_dropout = entity_dropout if entity_dropout else dropout            # model.py:953-954
        self.relation_dropout = relation_dropout if relation_dropout else dropout
        self.pool = "lstm"
        self.entity_projection = self.relation_projection = None
        self.entity_embedding_from_tokens = self.relations_embedding_from_tokens = None
        self.dropout_seed, self.dropout_step = seed, 0
        self._pool_engine = self._engine = None
        self._steps = []

    # -- plumbing ----------------------------------------------------------------------------------------------
    def _parts(self, relation):
        if relation:
            return self.relation_embedding, self.relation_token_ids, self.relation_encoder_in, self.relation_batchnorm
        return self.entity_embedding, self.entity_token_ids, self.entity_encoder_in, self.entity_batchnorm

    @staticmethod
    def _lstm_tensors(lstm):
        return [lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0]

    def _slot(self, relation, detach=True):
        emb, tok, lstm, bn = self._parts(relation)
        s = LSTMSlot.__new__(LSTMSlot)
        s.W, s.token_ids, s.d, s.L = emb.weight.detach(), tok.to(torch.int32).contiguous(), self.slot_size, tok.shape[1]
        s.lstm = [p.detach().contiguous() for p in self._lstm_tensors(lstm)]
        s.bn = None
        if bn is not None:
            s.bn = torch.cat([bn.weight.detach(), bn.bias.detach()])
            s.running_mean, s.running_var = bn.running_mean, bn.running_var
        return s

    def _encode(self, ids, relation, stream):
        """LSTM -> h at last -> batch-norm (batch statistics in training mode, running statistics otherwise) -> dropout"""
        eng = self.engine()
        ids = ids.reshape(-1).to(torch.int32).contiguous()
        n = ids.numel()
        emb, tok, lstm, bn = self._parts(relation)
        p = (self.relation_dropout if relation else self.entity_dropout) if self.training else 0.0
        params = [emb.weight] + self._lstm_tensors(lstm) + ([bn.weight, bn.bias] if bn is not None else [])
        if torch.is_grad_enabled() and any(q.requires_grad for q in params):
            from . import autograd_score as AG
            out = LSTMEncodeFn.apply(ids, self, relation, *params)
            if p > 0:
                out = AG.MaskRowsFn.apply(out, eng, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
            return out.unsqueeze(1)
        slot = self._slot(relation)
        raw = torch.empty((n, self.slot_size), device=ids.device)
        out = torch.empty_like(raw) if slot.bn is not None else raw
        if n:
            LstmPass(ids.device).encode(slot, [(ids, 0, n)], self.training, raw, out)
        if p > 0:
            out = eng.encode_rows(out, None, 0, n, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
        return out.unsqueeze(1)

    def precompute_embeddings_from_tokens(self):
        """model.py:670-712 (the reference encodes 4096 rows per call; any chunk size gives the same rows here)"""
        if self.entity_embedding_from_tokens is None:
            torch.nn.Module.train(self, False)         # the reference calls self.eval() here and stays in eval mode
            dev = self.entity_embedding.weight.device

            def table(n, relation):
                out = torch.empty((n, self.slot_size), device=dev)
                slot, ps = self._slot(relation), LstmPass(dev)
                for lo in range(0, n, PRECOMPUTE_CHUNK):
                    m = min(PRECOMPUTE_CHUNK, n - lo)
                    ps.encode(slot, [(None, lo, m)], False, out[lo:lo + m] if slot.bn is None else torch.empty((m, self.slot_size), device=dev),
                              out[lo:lo + m])
                return out
            with torch.no_grad():
                self.entity_embedding_from_tokens = table(self.train_data.entities_size, False)
                self.relations_embedding_from_tokens = table(self.train_data.relations_size, True)

    # -- AddLossModule / autograd bridge (the reference Trainer's path: trainer.py:142, 206-234) ---------------------
    def _lstm_slots(self, flat):
        """the two slots over the module's parameters; flat: the four LSTM tensors of each slot become views of one flat
        buffer (one optimizer segment)"""
        slots = []
        for relation in (False, True):
            emb, tok, lstm, bn = self._parts(relation)
            ps, buf = self._lstm_tensors(lstm), None
            if flat:
                buf = torch.cat([q.data.reshape(-1) for q in ps])
                for q, view in zip(ps, buf.split([q.numel() for q in ps])):
                    q.data = view.view_as(q)
            slots.append(LSTMSlot(emb.weight.data, tok, [q.data for q in ps], None if bn is None else (bn.weight.data, bn.bias.data),
                                  None if bn is None else (bn.running_mean, bn.running_var), flat=buf))
        return slots

    def autograd_step(self, loss, label_smoothing):
        """the cached LSTMTrainStep behind AddLossModule: shares the module's parameters; its optimizer is NOT used (the
        caller's torch optimizer steps the module parameters)"""
        st = getattr(self, "_ag_step", None)
        if st is None or st.loss != loss or st.label_smoothing != label_smoothing or st.entity.W.data_ptr() != self.entity_embedding.weight.data_ptr():
            slots = self._lstm_slots(flat=False)
            st = self._ag_step = LSTMTrainStep(slots[0], slots[1], self.scorer_name, loss=loss, label_smoothing=label_smoothing,
                                               dropout=self.entity_dropout, relation_dropout=self.relation_dropout, seed=self.dropout_seed)
        for sl, relation in ((st.entity, False), (st.relation, True)):
            emb, tok, lstm, bn = self._parts(relation)
            sl.lstm = [q.data for q in self._lstm_tensors(lstm)]             # (a torch optimizer may have replaced nothing, but
            sl.dW = torch.zeros_like(sl.W)                                     #  the gradient buffers went to autograd: fresh ones)
            sl.fresh_lstm_grads()
            if bn is not None:                                                 # the module's parameters may have been stepped outside
                sl.bn[:sl.d].copy_(bn.weight.data)
                sl.bn[sl.d:].copy_(bn.bias.data)
                sl.d_bn = torch.zeros_like(sl.d_bn)
        st.steps = self.dropout_step
        self.dropout_step += 1
        return st

    def autograd_params_and_grads(self, st):
        params, grads = [self.entity_embedding.weight, self.relation_embedding.weight], [st.entity.dW, st.relation.dW]
        for sl, relation in ((st.entity, False), (st.relation, True)):
            emb, tok, lstm, bn = self._parts(relation)
            if bn is not None:
                params += [bn.weight, bn.bias]
                grads += [sl.d_bn[:sl.d], sl.d_bn[sl.d:]]
            params += self._lstm_tensors(lstm)
            grads += sl.dlstm
        return params, grads

    def train_step(self, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8, label_smoothing=0.0):
        """The training driver for this model: shares the module's parameters (updated in place).  The four LSTM tensors of
        each slot become views of one flat buffer (one optimizer segment)."""
        slots = self._lstm_slots(flat=True)
        st = LSTMTrainStep(slots[0], slots[1], self.scorer_name, loss=loss, lr=lr, weight_decay=weight_decay, eps=eps,
                           label_smoothing=label_smoothing, dropout=self.entity_dropout, relation_dropout=self.relation_dropout,
                           seed=self.dropout_seed)
        if self.entity_batchnorm is not None:
            st.module_batchnorms = ((slots[0], self.entity_batchnorm), (slots[1], self.relation_batchnorm))
        return st


class LSTMComplexRelationModel(ComplexRelationScorer, LSTMRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


class LSTMDistmultRelationModel(DistmultRelationScorer, LSTMRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


# registered like the reference's (model.py:1052-1066): getattr(Models, args["model"])
Models.LSTMComplexRelationModel = LSTMComplexRelationModel
Models.LSTMDistmultRelationModel = LSTMDistmultRelationModel
