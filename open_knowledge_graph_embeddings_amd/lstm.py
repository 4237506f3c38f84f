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

import torch

from . import _native as N
from .model import ComplexRelationScorer, DistmultRelationScorer, Models
from .token_encoder import PRECOMPUTE_CHUNK, EncodeFn, EncoderPass, EncoderTrainStep, TokenEncoderEmbedder, bn_grad_pointers
from .token_embedder import BN_EPS, BN_MOMENTUM


class LstmPass(EncoderPass):
    """EncoderPass over okge_lstm_encode_calls / okge_lstm_backward_calls."""

    what, workspace_bytes = "LSTM", "okge_lstm_workspace_bytes"

    def encode(self, slot, calls, training, raw, out):
        """calls: [(ids int32 or None, first_id, n)] with n > 0, their rows one after the other in raw / out ([rows][ld])"""
        self._encode("okge_lstm_encode_calls", slot, calls, training, raw.data_ptr(), out.data_ptr(), raw.stride(0))

    def backward(self, slot, calls, raw, d_out, dW, dlstm, d_bn):
        """after encode(slot, calls, training=True, raw, ...): dW += token-row gradients; dlstm (4 tensors), d_bn ([w | b])
        are written"""
        pos, order = self._sorted_positions(slot)
        self._native("okge_lstm_backward_calls", slot, calls, raw.data_ptr(), d_out.data_ptr(), raw.stride(0), pos.data_ptr(),
                     order.data_ptr(), dW.data_ptr(), *(g.data_ptr() for g in dlstm), *bn_grad_pointers(slot, d_bn))


class LSTMSlot:
    """One embedder slot (entity or relation): token table, token-id matrix, the four nn.LSTM tensors, optional batch-norm,
    gradients and Adagrad accumulators."""

    what, has_raw, pass_class = "LSTM", True, LstmPass
    bn_calls = 0      # training-mode batch-norm encode calls of a train step since VirtualTableStep.sync_module (host count)

    def __init__(self, W, token_ids, lstm, bn=None, running=None, flat=None, view=False):
        """lstm: [weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0]; bn: [weight, bias] or None; running: (mean, var);
        flat: one buffer the four LSTM tensors are views of (one optimizer segment instead of four), or None;
        view: a slot to encode with (and to run a backward into the caller's buffers): no gradient or accumulator buffers"""
        self.W, self.token_ids = W, token_ids.to(torch.int32).contiguous()
        self.d, self.L = W.shape[1], self.token_ids.shape[1]
        self.lstm, self.flat = list(lstm), flat
        dev = W.device
        self.bn = None
        if bn is not None:
            self.bn = torch.cat([bn[0].reshape(-1), bn[1].reshape(-1)]).to(device=dev, dtype=torch.float32).contiguous()
            self.running_mean, self.running_var = running
        if view:
            return
        self.dW = torch.zeros_like(W)
        self.sumW = torch.zeros_like(W)
        self.fresh_grads()
        self.sum_flat = torch.zeros_like(self.d_flat)
        if bn is not None:
            self.sum_bn = torch.zeros_like(self.d_bn)

    def fresh_grads(self):
        """d_flat: one zeroed gradient buffer; dlstm: the four LSTM tensors' gradients as views of it; d_bn ([w | b])"""
        self.d_flat = torch.zeros(sum(p.numel() for p in self.lstm), dtype=torch.float32, device=self.W.device)
        self.dlstm = [g.view_as(p) for g, p in zip(self.d_flat.split([p.numel() for p in self.lstm]), self.lstm)]
        if self.bn is not None:
            self.d_bn = torch.zeros_like(self.bn)

    def encoder_grads(self):
        dl = [torch.empty_like(p) for p in self.lstm]
        return dl, dl

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


class LSTMTrainStep(EncoderTrainStep):
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

    def __init__(self, entity: LSTMSlot, relation: LSTMSlot, scorer, *args, **kwargs):
        super().__init__(entity, relation, scorer, *args, **kwargs)
        self.relation_unused = scorer == "bias_entity"

    def _unused(self, sl):
        return self.relation_unused and sl is self.relation

    @staticmethod
    def _bn_state(sl):
        return [sl.bn, sl.d_bn, sl.sum_bn, sl.running_mean, sl.running_var]

    def _encode_slot(self, ps, sl, calls, V, X):
        if not self._unused(sl) or sl.bn is not None:                     # (unused: only for the running statistics)
            ps.encode(sl, calls, True, X, V)
            if sl.bn is not None:
                sl.bn_calls += len(calls)

    def _backward_slot(self, ps, sl, calls, X, dV):
        """batch-norm and the LSTM backward through time -> the slot's dW, d_flat (dlstm), d_bn ([d weight | d bias])"""
        if not self._unused(sl):
            ps.backward(sl, calls, X, dV, sl.dW, sl.dlstm, sl.d_bn if sl.bn is not None else None)

    def optimizer_step(self):
        self._update(self._param_groups())                         # (up to four tensors per launch; an unused relation slot: none)
        self._sync_module_batchnorms()


LSTMEncodeFn = EncodeFn                            # (the shared Function: LSTMSlot says what its encode takes)


# ------------------------------------------------------------------------------------------------------------------
# API-compatible model classes
# ------------------------------------------------------------------------------------------------------------------
class LSTMRelationEmbedder(TokenEncoderEmbedder):
    """openkge/model.py:912-998.  Implemented: normalize None|''|'batchnorm', dropout / entity_dropout / relation_dropout
    (Philox masks), slot sizes up to 512; not implemented (raise at construction): encoder_activiation, project_relation,
    sparse, relation_slot_size != entity_slot_size.  Training: LSTMTrainStep (fused, own dense Adagrad) or
    trainer.AddLossModule (autograd bridge: any torch optimizer over the module's parameters)."""

    what, _train_step_class = "LSTM", LSTMTrainStep

    def __init__(self, entity_slot_size, relation_slot_size, train_data, dropout=0.0, entity_dropout=None, relation_dropout=None,
                 encoder_activiation=None, sparse=False, init_std=0.1, normalize='', project_relation=False, seed=0):
        super().__init__()
        relation_slot_size = self._refuse_unsupported(entity_slot_size, relation_slot_size, encoder_activiation, project_relation, sparse)
        if normalize not in (None, '', 'batchnorm'):
            raise NotImplementedError(f"normalize={normalize!r}")
        self._init_token_tables(train_data, entity_slot_size, normalize, init_std)             # then model.py:932-952
        # (nn.LSTM warns that dropout has no effect on one layer; kept as the reference passes it)
        self.entity_encoder_in = torch.nn.LSTM(input_size=entity_slot_size, hidden_size=entity_slot_size, batch_first=True, dropout=dropout)
        self.relation_encoder_in = torch.nn.LSTM(input_size=relation_slot_size, hidden_size=relation_slot_size, batch_first=True,
                                                 dropout=dropout)
        self.pool = "lstm"
        self._init_state(dropout, entity_dropout, relation_dropout, seed)

    # -- plumbing ----------------------------------------------------------------------------------------------
    def _parts(self, relation):
        if relation:
            return self.relation_embedding, self.relation_token_ids, self.relation_encoder_in, self.relation_batchnorm
        return self.entity_embedding, self.entity_token_ids, self.entity_encoder_in, self.entity_batchnorm

    @staticmethod
    def _lstm_tensors(lstm):
        return [lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0]

    def _params(self, relation):
        emb, tok, lstm, bn = self._parts(relation)
        return [emb.weight] + self._lstm_tensors(lstm) + ([bn.weight, bn.bias] if bn is not None else [])

    def _slot(self, relation):
        """a view slot over the module's current parameters"""
        emb, tok, lstm, bn = self._parts(relation)
        return LSTMSlot(emb.weight.detach(), tok, [p.detach().contiguous() for p in self._lstm_tensors(lstm)],
                        None if bn is None else (bn.weight.detach(), bn.bias.detach()),
                        None if bn is None else (bn.running_mean, bn.running_var), view=True)

    @staticmethod
    def _precompute_chunk():
        return PRECOMPUTE_CHUNK                        # (this module's: a test shrinks it)

    # -- AddLossModule / autograd bridge (the reference Trainer's path: trainer.py:142, 206-234) ---------------------
    def _train_slots(self, flat=True):
        """the two slots over the module's parameters; flat (train_step()): the four LSTM tensors of each slot become views
        of one flat buffer (one optimizer segment)"""
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
        st = self._cached_autograd_step(loss, label_smoothing, lambda: self._train_slots(flat=False))
        for sl, relation in ((st.entity, False), (st.relation, True)):
            sl.lstm = [q.data for q in self._lstm_tensors(self._parts(relation)[2])]
        return self._refresh_autograd_step(st)

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

    def _state_segments(self, sl, relation):
        """optimizer_params_and_state: the token table, the four LSTM tensors one after the other in the slot's flat buffer, the
        batch-norm's [weight | bias]"""
        emb, tok, lstm, bn = self._parts(relation)
        out, offset = [(emb.weight, (sl.W, sl.sumW), 0)], 0
        for q in self._lstm_tensors(lstm):
            out.append((q, (sl.flat, sl.sum_flat), offset))
            offset += q.numel()
        if bn is not None:
            out += [(bn.weight, (sl.bn, sl.sum_bn), 0), (bn.bias, (sl.bn, sl.sum_bn), sl.d)]
        return out


class LSTMComplexRelationModel(ComplexRelationScorer, LSTMRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


class LSTMDistmultRelationModel(DistmultRelationScorer, LSTMRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


# registered like the reference's (model.py:1052-1066): getattr(Models, args["model"])
Models.LSTMComplexRelationModel = LSTMComplexRelationModel
Models.LSTMDistmultRelationModel = LSTMDistmultRelationModel
