"""Bigram-pooling embedder: BigramPoolingRelationEmbedder + BigramPooling{Complex,Distmult}RelationModel (openkge/model.py:
801-909, :1021-1024) over the HIP kernels of csrc/okge_bigram.hip (the pair product on the exact-fp32 MFMA, forward and
backward), and the training step that drives the fused prefix-scoring path on rows encoded from tokens.

The reference's encode_subj / encode_obj / encode_rel hand ids to `_encode`, which treats them as a token matrix: the class
raises as shipped.  The evident intent -- tokens = entity_token_ids[ids] first -- is what this module does; every parity
statement is against the reference run through a shim that does exactly that mapping around its unmodified `encode_*`.

normalize='batchnorm' here is NOT the unigram / LSTM batch-norm: it is a BatchNorm1d(d, momentum=None) inside the encoder,
over the convolution output at all n (L-1) positions of a call, padded positions included; running statistics are a cumulative
average.  So the virtual-table step sees finished rows: the skeleton reads EV for a batch-normed slot and EX otherwise, and
`_encode` writes the encoded rows there.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N
from . import hotpath as H
from .model import ComplexRelationScorer, DistmultRelationScorer, Models
from . import virtual_tables as VT
from .token_pooled import BN_EPS, UnigramPoolingRelationEmbedder, token_id_matrix

MAX_SLOT = 512                                     # the fused tile kernels' largest slot size
MAX_LEN = 64
PRECOMPUTE_CHUNK = 16384                           # rows per encode call of precompute_embeddings_from_tokens
POOL_SUM, POOL_MAX = 0, 1
NORM_NONE, NORM_MEAN, NORM_BATCHNORM = 0, 1, 2


def pool_code(pool):
    return POOL_MAX if pool == 'max' else POOL_SUM         # model.py:883-886: any pool other than 'max' sums


def norm_code(normalize):
    return {'mean': NORM_MEAN, 'batchnorm': NORM_BATCHNORM}.get(normalize, NORM_NONE)


class BigramSlot:
    """One embedder slot (entity or relation): token table, token-id matrix, the Conv1d weight (d, d, 2), optional batch-norm
    (weight, bias, running statistics, num_batches_tracked), gradients and Adagrad accumulators.  conv weight and batch-norm
    parameters are views of one flat buffer [conv | bn weight | bn bias] (one optimizer segment)."""

    def __init__(self, W, token_ids, conv, pool='', normalize='', bn=None, running=None, num_batches_tracked=None):
        """conv: (d, d, 2); bn: (weight, bias) with normalize='batchnorm'; running: (mean, var) or None (fresh)"""
        self.W, self.token_ids = W, token_ids.to(torch.int32).contiguous()
        self.d, self.L = W.shape[1], self.token_ids.shape[1]
        self.pool, self.normalize = pool, normalize
        d, dev = self.d, W.device
        batchnorm = normalize == 'batchnorm'
        parts = [conv.reshape(-1)] + ([bn[0].reshape(-1), bn[1].reshape(-1)] if batchnorm else [])
        self.flat = torch.cat(parts).to(device=dev, dtype=torch.float32).contiguous()
        self.sum_flat = torch.zeros_like(self.flat)
        self.dW = torch.zeros_like(W)
        self.sumW = torch.zeros_like(W)
        self.bn = None
        if batchnorm:
            self.running_mean, self.running_var = running if running is not None else \
                (torch.zeros(d, device=dev), torch.ones(d, device=dev))
            self.num_batches_tracked = num_batches_tracked if num_batches_tracked is not None else \
                torch.zeros((), dtype=torch.int64, device=dev)
        self.bind()
        self.fresh_grads()

    def bind(self):
        """conv / bn: views of flat"""
        d = self.d
        self.conv = self.flat[:2 * d * d].view(d, d, 2)
        self.bn = self.flat[2 * d * d:] if self.normalize == 'batchnorm' else None

    def fresh_grads(self):
        """d_flat: one zeroed gradient buffer; d_conv, d_bn: views of it"""
        d = self.d
        self.d_flat = torch.zeros_like(self.flat)
        self.d_conv = self.d_flat[:2 * d * d].view(d, d, 2)
        self.d_bn = self.d_flat[2 * d * d:] if self.bn is not None else None

    def c(self):
        s = N.BigramSlot()
        s.W, s.token_ids = self.W.data_ptr(), self.token_ids.data_ptr()
        s.vocab, s.d, s.n_ids, s.max_len = self.W.shape[0], self.d, self.token_ids.shape[0], self.L
        s.conv_weight, s.pool, s.normalize = self.conv.data_ptr(), pool_code(self.pool), norm_code(self.normalize)
        if self.bn is not None:
            s.bn_weight, s.bn_bias = self.bn[:self.d].data_ptr(), self.bn[self.d:].data_ptr()
            s.bn_running_mean, s.bn_running_var = self.running_mean.data_ptr(), self.running_var.data_ptr()
            s.bn_num_batches_tracked, s.bn_eps = self.num_batches_tracked.data_ptr(), BN_EPS
        return s

    def optimizer_tensors(self):
        return [(self.W, self.dW, self.sumW), (self.flat, self.d_flat, self.sum_flat)]


class BigramPass:
    """The workspace of one bigram pass (a slot's calls of one step) and its ctypes driver (okge_bigram_encode_calls /
    okge_bigram_backward_calls).  A backward needs the workspace its forward left: one object per pass in flight."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.lib = N.lib()
        self.ws, self.ws_bytes = None, 0
        self.pos_tok = None
        self.rows, self.trained = 0, False

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _calls(self, calls):
        arr = (N.BigramCall * len(calls))()
        for x, (ids, first_id, n) in zip(arr, calls):
            x.ids, x.first_id, x.n = None if ids is None else ids.data_ptr(), int(first_id), int(n)
        return arr

    def encode(self, slot: BigramSlot, calls, training, out):
        """calls: [(ids int32 or None, first_id, n)] with n > 0, their rows one after the other in out ([rows][ld])"""
        rows = sum(int(c[2]) for c in calls)
        need = int(self.lib.okge_bigram_workspace_bytes(rows, slot.L, slot.d, int(bool(training))))
        if need > self.ws_bytes:
            self.ws, self.ws_bytes = torch.empty(need, dtype=torch.uint8, device=self.device), need
        if self.pos_tok is None or self.pos_tok.numel() < rows * slot.L:
            self.pos_tok = torch.empty(max(rows * slot.L, 1), dtype=torch.int32, device=self.device)
        self.rows, self.trained = rows, False
        s = slot.c()
        N.check(self.lib.okge_bigram_encode_calls(ctypes.byref(s), self._calls(calls), len(calls), int(bool(training)), out.data_ptr(),
                                                  out.stride(0), self.pos_tok.data_ptr(), 0 if self.ws is None else self.ws.data_ptr(),
                                                  self.ws_bytes, self._stream()), "okge_bigram_encode_calls")
        self.trained = bool(training)

    def backward(self, slot: BigramSlot, calls, d_out, dW, d_conv, d_bn):
        """after encode(slot, calls, training=True, ...): dW += token-row gradients; d_conv (d, d, 2) and d_bn ([w | b]) are
        written"""
        if not self.trained:
            raise RuntimeError("bigram backward without a training-mode forward")
        pos = self.pos_tok[:self.rows * slot.L]
        order = torch.argsort(pos, stable=True).to(torch.int32)           # (index plumbing; the sums are the kernel's)
        s = slot.c()
        d = slot.d
        bn = slot.bn is not None
        N.check(self.lib.okge_bigram_backward_calls(ctypes.byref(s), self._calls(calls), len(calls), d_out.data_ptr(), d_out.stride(0),
                                                    pos.data_ptr(), order.data_ptr(), dW.data_ptr(), d_conv.data_ptr(),
                                                    d_bn[:d].data_ptr() if bn else None, d_bn[d:].data_ptr() if bn else None,
                                                    self.ws.data_ptr(), self.ws_bytes, self._stream()), "okge_bigram_backward_calls")


class BigramTrainStep(VT.VirtualTableStep):
    """forward + loss + backward + Adagrad for BigramPooling{Complex,Distmult}RelationModel (Trainer.compute_one_batch,
    trainer.py:181-257, over model.py:874-906 with the id -> token mapping).  The optimizer is dense: every token row, the
    conv weight and the batch-norm parameters move every step (utils/optim.py:139-160).  Deferred decay, ReplicaStep sharding
    and graph capture are not implemented for this step."""

    def __init__(self, entity: BigramSlot, relation: BigramSlot, scorer, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8,
                 label_smoothing=0.0, dropout=0.0, relation_dropout=None, seed=0, engine=None):
        super().__init__(entity, relation, scorer, loss=loss, lr=lr, weight_decay=weight_decay, eps=eps,
                         label_smoothing=label_smoothing, dropout=dropout, relation_dropout=relation_dropout, seed=seed, engine=engine)
        self.passes = (BigramPass(self.device), BigramPass(self.device))
        self.decay_window = 1

    def state_tensors(self):
        out = []
        for sl in (self.entity, self.relation):
            out += [sl.W, sl.dW, sl.sumW, sl.flat, sl.d_flat, sl.sum_flat]
            if sl.bn is not None:
                out += [sl.running_mean, sl.running_var, sl.num_batches_tracked]
        return out

    def flush(self):
        """(no deferred updates here: every parameter is current after every step)"""

    @staticmethod
    def _rows(sl, V, X):
        """the buffer the skeleton hands to the fused step for this slot: the encoder's output IS the finished row"""
        return V if sl.bn is not None else X

    def _encode(self, batch: H.PrefixBatch, bufs):
        """one bigram pass per slot over its calls, in the reference's encode order; -> the two slots' non-empty calls"""
        dev = self.device
        EV, EX, dEV, RV, RX, dRV = bufs
        calls = ([], [])
        for relation, ids, first, rows in VT.encode_calls(batch):
            if rows.stop > rows.start:
                calls[relation].append((H._i32(ids, dev), first, rows.stop - rows.start))
        self.passes[0].encode(self.entity, calls[0], True, self._rows(self.entity, EV, EX))
        self.passes[1].encode(self.relation, calls[1], True, self._rows(self.relation, RV, RX))
        return calls

    def _backward(self, batch, bufs, calls):
        """dEV / dRV -> pooling, batch-norm and the pair product's backward -> the slots' dW, d_flat ([d conv | d bn])"""
        EV, EX, dEV, RV, RX, dRV = bufs
        for ps, sl, cs, dV in zip(self.passes, (self.entity, self.relation), calls, (dEV, dRV)):
            ps.backward(sl, cs, dV, sl.dW, sl.d_conv, sl.d_bn)

    def optimizer_step(self):
        self.engine.adagrad_multi(self.entity.optimizer_tensors() + self.relation.optimizer_tensors(), self.lr, self.weight_decay, self.eps)


class BigramEncodeFn(torch.autograd.Function):
    """encode_* with gradients enabled (a caller's own loss): the HIP forward and backward of ONE call, with a workspace of
    its own (kept until backward).  Inputs after the first three are the slot's parameters, so that autograd hands their
    gradients on: W, conv weight[, bn weight, bn bias]."""

    @staticmethod
    def forward(ctx, ids, module, relation, W, conv, *bn):
        slot = module._slot(relation)
        n = ids.numel()
        out = torch.empty((n, slot.d), device=ids.device)
        ps = BigramPass(ids.device)
        training = module.training
        ps.encode(slot, [(ids, 0, n)], training, out)
        ctx.slot, ctx.ps, ctx.ids, ctx.training = slot, ps, ids, training
        return out

    @staticmethod
    def backward(ctx, g):
        if not ctx.training:
            raise RuntimeError("gradients of an eval-mode bigram encode are not implemented")
        slot = ctx.slot
        d = slot.d
        dW = torch.zeros_like(slot.W)
        d_conv = torch.empty_like(slot.conv)
        d_bn = torch.empty(2 * d, device=g.device) if slot.bn is not None else None
        ctx.ps.backward(slot, [(ctx.ids, 0, ctx.ids.numel())], g.contiguous(), dW, d_conv, d_bn)
        bn_grads = () if d_bn is None else (d_bn[:d].clone(), d_bn[d:].clone())
        return (None, None, None, dW, d_conv, *bn_grads)


# ------------------------------------------------------------------------------------------------------------------
# API-compatible model classes
# ------------------------------------------------------------------------------------------------------------------
class BigramPoolingRelationEmbedder(UnigramPoolingRelationEmbedder):
    """openkge/model.py:801-909, with the id -> token mapping its encode_* leave out.  Implemented: normalize
    '' | None | 'mean' | 'batchnorm', pool 'max' or anything else (= sum), dropout / entity_dropout / relation_dropout (Philox
    masks), slot sizes up to 512, max_length 2..64; not implemented (raise at construction): gates=True, normalize='norm',
    encoder_activiation, project_relation, sparse, unequal slot sizes, slot sizes above 512, max_length below 2.  Training:
    BigramTrainStep (fused, own dense Adagrad) or trainer.AddLossModule (autograd bridge: any torch optimizer over the
    module's parameters).  The evaluation surface (get_all_* / get_*, prefix scores, loss_only) is the token-pooled
    embedder's."""

    def __init__(self, entity_slot_size, relation_slot_size, train_data, normalize='', pool='', dropout=0.0, entity_dropout=None,
                 relation_dropout=None, encoder_activiation=None, sparse=False, init_std=0.01, gates=False, project_relation=False,
                 seed=0):
        torch.nn.Module.__init__(self)
        if relation_slot_size is None or relation_slot_size <= 0:
            relation_slot_size = entity_slot_size
        if gates:
            raise NotImplementedError("gates=True is not implemented for the bigram embedder")
        if normalize == 'norm':
            raise NotImplementedError("normalize='norm' is not implemented for the bigram embedder")
        if encoder_activiation is not None:
            raise NotImplementedError("encoder_activiation is not implemented for the bigram embedder")
        if project_relation:
            raise NotImplementedError("project_relation is not implemented for the bigram embedder")
        if sparse:
            raise NotImplementedError("sparse gradients are not implemented for the bigram embedder")
        if relation_slot_size != entity_slot_size:
            raise NotImplementedError("unequal slot sizes: the relation slot size must equal the entity slot size")
        if entity_slot_size > MAX_SLOT:
            raise NotImplementedError(f"bigram slot sizes above {MAX_SLOT}")
        max_len = train_data.max_length
        e_len, r_len = (max_len, max_len) if isinstance(max_len, int) else (max_len[0], max_len[1])
        if min(e_len, r_len) < 2:
            raise NotImplementedError("max_length below 2: a bigram needs two token positions")
        if max(e_len, r_len) > MAX_LEN:
            raise NotImplementedError(f"max_length above {MAX_LEN}")
        self.train_data, self.slot_size, self.relation_slot_size = train_data, entity_slot_size, relation_slot_size
        self.normalize, self.pool, self.gates = normalize, pool, False
        d = entity_slot_size
        # the reference's constructor order (TokenBasedRelationEmbedder.__init__, model.py:568-634, then :856-872): the same
        # torch.manual_seed gives bit-identical initial parameters.  The base class draws uniform_ weights for batch-norm
        # modules that this class then replaces: the draws are kept (they move the generator), the modules are not.
        self.register_buffer('entity_token_ids', token_id_matrix(train_data.entity_id_to_tokens_map, e_len))
        self.register_buffer('relation_token_ids', token_id_matrix(train_data.relation_id_to_tokens_map, r_len))
        self.entity_embedding = torch.nn.Embedding(train_data.entity_tokens_size, d, padding_idx=0)
        self.relation_embedding = torch.nn.Embedding(train_data.relation_tokens_size, d, padding_idx=0)
        self.entity_batchnorm = self.relation_batchnorm = None
        if normalize == 'batchnorm':
            self.entity_batchnorm = torch.nn.BatchNorm1d(d, momentum=0.1, eps=BN_EPS)
            self.relation_batchnorm = torch.nn.BatchNorm1d(d, momentum=0.1, eps=BN_EPS)
            torch.nn.init.uniform_(self.entity_batchnorm.weight)
            torch.nn.init.uniform_(self.relation_batchnorm.weight)
        torch.nn.init.normal_(self.entity_embedding.weight.data, std=init_std)          # row 0 included
        torch.nn.init.normal_(self.relation_embedding.weight.data, std=init_std)
        self.entity_batchnorm = self.relation_batchnorm = None      # (registered names keep their place in the module order)
        if normalize == 'batchnorm':
            self.entity_batchnorm = torch.nn.BatchNorm1d(d, momentum=None)
            self.relation_batchnorm = torch.nn.BatchNorm1d(d, momentum=None)
        # real torch modules as parameter storage, composed as the reference composes them (state_dict lists the batch-norm
        # under both entity_batchnorm.* and entity_encoder_in.1.*); their forward is never called
        self.entity_encoder_in = torch.nn.Sequential(
            torch.nn.Conv1d(in_channels=d, out_channels=d, kernel_size=2, dilation=1, bias=False),
            *([self.entity_batchnorm] if self.entity_batchnorm is not None else []))
        self.relation_encoder_in = torch.nn.Sequential(
            torch.nn.Conv1d(in_channels=d, out_channels=d, kernel_size=2, dilation=1, bias=False),
            *([self.relation_batchnorm] if self.relation_batchnorm is not None else []))
        self.entity_dropout = entity_dropout if entity_dropout else dropout            # model.py:845-846
        self.relation_dropout = relation_dropout if relation_dropout else dropout
        self.entity_projection = self.relation_projection = None
        self.entity_embedding_from_tokens = self.relations_embedding_from_tokens = None
        self.dropout_seed, self.dropout_step = seed, 0
        self._pool_engine = self._engine = None
        self._steps = []

    # -- plumbing ----------------------------------------------------------------------------------------------
    def _parts(self, relation):
        if relation:
            return self.relation_embedding, self.relation_token_ids, self.relation_encoder_in[0], self.relation_batchnorm
        return self.entity_embedding, self.entity_token_ids, self.entity_encoder_in[0], self.entity_batchnorm

    def _params(self, relation):
        emb, tok, conv, bn = self._parts(relation)
        return [emb.weight, conv.weight] + ([bn.weight, bn.bias] if bn is not None else [])

    def _slot(self, relation):
        """a slot over the module's current parameters (copies of conv / batch-norm parameters in the slot's flat buffer; the
        token table, running statistics and counter are the module's own tensors)"""
        emb, tok, conv, bn = self._parts(relation)
        return BigramSlot(emb.weight.detach(), tok, conv.weight.detach(), self.pool, self.normalize,
                          None if bn is None else (bn.weight.detach(), bn.bias.detach()),
                          None if bn is None else (bn.running_mean, bn.running_var), None if bn is None else bn.num_batches_tracked)

    def _encode(self, ids, relation, stream):
        """tokens of the ids -> pair convolution -> [batch-norm over positions] -> residual, mask, pool[, mean] -> dropout"""
        eng = self.engine()
        ids = ids.reshape(-1).to(torch.int32).contiguous()
        n = ids.numel()
        p = (self.relation_dropout if relation else self.entity_dropout) if self.training else 0.0
        params = self._params(relation)
        if torch.is_grad_enabled() and any(q.requires_grad for q in params):
            from . import autograd_score as AG
            out = BigramEncodeFn.apply(ids, self, relation, *params)
            if p > 0:
                out = AG.MaskRowsFn.apply(out, eng, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
            return out.unsqueeze(1)
        out = torch.empty((n, self.slot_size), device=ids.device)
        if n:
            BigramPass(ids.device).encode(self._slot(relation), [(ids, 0, n)], self.training, out)
        if p > 0:
            out = eng.encode_rows(out, None, 0, n, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
        return out.unsqueeze(1)

    def precompute_embeddings_from_tokens(self):
        """model.py:670-712 (the reference encodes 4096 rows per call; in eval mode any chunk size gives the same rows)"""
        if self.entity_embedding_from_tokens is None:
            torch.nn.Module.train(self, False)         # the reference calls self.eval() here and stays in eval mode
            dev = self.entity_embedding.weight.device

            def table(n, relation):
                out = torch.empty((n, self.slot_size), device=dev)
                slot, ps = self._slot(relation), BigramPass(dev)
                for lo in range(0, n, PRECOMPUTE_CHUNK):
                    m = min(PRECOMPUTE_CHUNK, n - lo)
                    ps.encode(slot, [(None, lo, m)], False, out[lo:lo + m])
                return out
            with torch.no_grad():
                self.entity_embedding_from_tokens = table(self.train_data.entities_size, False)
                self.relations_embedding_from_tokens = table(self.train_data.relations_size, True)

    # -- AddLossModule / autograd bridge (the reference Trainer's path: trainer.py:142, 206-234) ---------------------
    def _bigram_slots(self, share):
        """the two slots over the module's parameters; share: conv weight and batch-norm parameters of the module become
        views of the slot's flat buffer (an optimizer step on the slot moves the module)"""
        slots = []
        for relation in (False, True):
            emb, tok, conv, bn = self._parts(relation)
            sl = BigramSlot(emb.weight.data, tok, conv.weight.data, self.pool, self.normalize,
                            None if bn is None else (bn.weight.data, bn.bias.data),
                            None if bn is None else (bn.running_mean, bn.running_var), None if bn is None else bn.num_batches_tracked)
            if share:
                conv.weight.data = sl.conv
                if bn is not None:
                    bn.weight.data, bn.bias.data = sl.bn[:sl.d], sl.bn[sl.d:]
            slots.append(sl)
        return slots

    def autograd_step(self, loss, label_smoothing):
        """the cached BigramTrainStep behind AddLossModule: reads the module's parameters; its optimizer is NOT used (the
        caller's torch optimizer steps the module parameters)"""
        st = getattr(self, "_ag_step", None)
        if st is None or st.loss != loss or st.label_smoothing != label_smoothing or st.entity.W.data_ptr() != self.entity_embedding.weight.data_ptr():
            slots = self._bigram_slots(share=False)
            st = self._ag_step = BigramTrainStep(slots[0], slots[1], self.scorer_name, loss=loss, label_smoothing=label_smoothing,
                                                 dropout=self.entity_dropout, relation_dropout=self.relation_dropout, seed=self.dropout_seed)
        for sl, relation in ((st.entity, False), (st.relation, True)):
            emb, tok, conv, bn = self._parts(relation)
            sl.conv.copy_(conv.weight.data)                                    # the module's parameters may have been stepped outside
            if bn is not None:
                sl.bn[:sl.d].copy_(bn.weight.data)
                sl.bn[sl.d:].copy_(bn.bias.data)
                sl.running_mean, sl.running_var, sl.num_batches_tracked = bn.running_mean, bn.running_var, bn.num_batches_tracked
            sl.dW = torch.zeros_like(sl.W)                                     # fresh gradient buffers: the last ones went to autograd
            sl.fresh_grads()
        st.steps = self.dropout_step
        self.dropout_step += 1
        return st

    def autograd_params_and_grads(self, st):
        params, grads = [], []
        for sl, relation in ((st.entity, False), (st.relation, True)):
            params += self._params(relation)
            grads += [sl.dW, sl.d_conv] + ([sl.d_bn[:sl.d], sl.d_bn[sl.d:]] if sl.bn is not None else [])
        return params, grads

    def train_step(self, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8, label_smoothing=0.0):
        """The training driver for this model: shares the module's parameters (updated in place).  The conv weight and the
        batch-norm parameters of each slot become views of one flat buffer (one optimizer segment)."""
        slots = self._bigram_slots(share=True)
        return BigramTrainStep(slots[0], slots[1], self.scorer_name, loss=loss, lr=lr, weight_decay=weight_decay, eps=eps,
                               label_smoothing=label_smoothing, dropout=self.entity_dropout, relation_dropout=self.relation_dropout,
                               seed=self.dropout_seed)


class BigramPoolingComplexRelationModel(ComplexRelationScorer, BigramPoolingRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


class BigramPoolingDistmultRelationModel(DistmultRelationScorer, BigramPoolingRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


# registered like the reference's (model.py:1052-1066): getattr(Models, args["model"])
Models.BigramPoolingComplexRelationModel = BigramPoolingComplexRelationModel
Models.BigramPoolingDistmultRelationModel = BigramPoolingDistmultRelationModel
