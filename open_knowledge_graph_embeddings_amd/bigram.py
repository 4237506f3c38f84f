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

import torch

from . import _native as N
from .model import ComplexRelationScorer, DistmultRelationScorer, Models
from .token_encoder import PRECOMPUTE_CHUNK, EncodeFn, EncoderPass, EncoderTrainStep, TokenEncoderEmbedder, bn_grad_pointers
from .token_embedder import BN_EPS

MAX_LEN = 64
POOL_SUM, POOL_MAX = 0, 1
NORM_NONE, NORM_MEAN, NORM_BATCHNORM = 0, 1, 2


def pool_code(pool):
    return POOL_MAX if pool == 'max' else POOL_SUM         # model.py:883-886: any pool other than 'max' sums


def norm_code(normalize):
    return {'mean': NORM_MEAN, 'batchnorm': NORM_BATCHNORM}.get(normalize, NORM_NONE)


class BigramPass(EncoderPass):
    """EncoderPass over okge_bigram_encode_calls / okge_bigram_backward_calls."""

    what, workspace_bytes = "bigram", "okge_bigram_workspace_bytes"

    def encode(self, slot, calls, training, out):
        """calls: [(ids int32 or None, first_id, n)] with n > 0, their rows one after the other in out ([rows][ld])"""
        self._encode("okge_bigram_encode_calls", slot, calls, training, out.data_ptr(), out.stride(0))

    def backward(self, slot, calls, d_out, dW, d_conv, d_bn):
        """after encode(slot, calls, training=True, ...): dW += token-row gradients; d_conv (d, d, 2) and d_bn ([w | b]) are
        written"""
        pos, order = self._sorted_positions(slot)
        self._native("okge_bigram_backward_calls", slot, calls, d_out.data_ptr(), d_out.stride(0), pos.data_ptr(), order.data_ptr(),
                     dW.data_ptr(), d_conv.data_ptr(), *bn_grad_pointers(slot, d_bn))


class BigramSlot:
    """One embedder slot (entity or relation): token table, token-id matrix, the Conv1d weight (d, d, 2), optional batch-norm
    (weight, bias, running statistics, num_batches_tracked), gradients and Adagrad accumulators.  conv weight and batch-norm
    parameters are views of one flat buffer [conv | bn weight | bn bias] (one optimizer segment)."""

    what, has_raw, pass_class = "bigram", False, BigramPass

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

    def encoder_grads(self):
        g = torch.empty_like(self.conv)
        return g, [g]

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


class BigramTrainStep(EncoderTrainStep):
    """forward + loss + backward + Adagrad for BigramPooling{Complex,Distmult}RelationModel (Trainer.compute_one_batch,
    trainer.py:181-257, over model.py:874-906 with the id -> token mapping).  The optimizer is dense: every token row, the
    conv weight and the batch-norm parameters move every step (utils/optim.py:139-160).  Deferred decay, ReplicaStep sharding
    and graph capture are not implemented for this step."""

    @staticmethod
    def _bn_state(sl):
        return [sl.running_mean, sl.running_var, sl.num_batches_tracked]

    @staticmethod
    def _rows(sl, V, X):
        """the buffer the skeleton hands to the fused step for this slot: the encoder's output IS the finished row"""
        return V if sl.bn is not None else X

    def _encode_slot(self, ps, sl, calls, V, X):
        ps.encode(sl, calls, True, self._rows(sl, V, X))

    def _backward_slot(self, ps, sl, calls, X, dV):
        """pooling, batch-norm and the pair product's backward -> the slot's dW, d_flat ([d conv | d bn])"""
        ps.backward(sl, calls, dV, sl.dW, sl.d_conv, sl.d_bn)

    def optimizer_step(self):
        self._update(self._param_groups())


BigramEncodeFn = EncodeFn                          # (the shared Function: BigramSlot says what its encode takes)


# ------------------------------------------------------------------------------------------------------------------
# API-compatible model classes
# ------------------------------------------------------------------------------------------------------------------
class BigramPoolingRelationEmbedder(TokenEncoderEmbedder):
    """openkge/model.py:801-909, with the id -> token mapping its encode_* leave out.  Implemented: normalize
    '' | None | 'mean' | 'batchnorm', pool 'max' or anything else (= sum), dropout / entity_dropout / relation_dropout (Philox
    masks), slot sizes up to 512, max_length 2..64; not implemented (raise at construction): gates=True, normalize='norm',
    encoder_activiation, project_relation, sparse, unequal slot sizes, slot sizes above 512, max_length below 2.  Training:
    BigramTrainStep (fused, own dense Adagrad) or trainer.AddLossModule (autograd bridge: any torch optimizer over the
    module's parameters)."""

    what, _train_step_class = "bigram", BigramTrainStep
    step_copies_batchnorm = False      # (train_step(): the module's batch-norm parameters ARE views of the slots' buffers)

    def __init__(self, entity_slot_size, relation_slot_size, train_data, normalize='', pool='', dropout=0.0, entity_dropout=None,
                 relation_dropout=None, encoder_activiation=None, sparse=False, init_std=0.01, gates=False, project_relation=False,
                 seed=0):
        super().__init__()
        if gates:
            raise NotImplementedError("gates=True is not implemented for the bigram embedder")
        if normalize == 'norm':
            raise NotImplementedError("normalize='norm' is not implemented for the bigram embedder")
        self._refuse_unsupported(entity_slot_size, relation_slot_size, encoder_activiation, project_relation, sparse)
        e_len, r_len = self._max_lengths(train_data)
        if min(e_len, r_len) < 2:
            raise NotImplementedError("max_length below 2: a bigram needs two token positions")
        if max(e_len, r_len) > MAX_LEN:
            raise NotImplementedError(f"max_length above {MAX_LEN}")
        self.pool, self.gates = pool, False
        d = entity_slot_size
        # then model.py:856-872.  The base class draws uniform_ weights for batch-norm modules that this class then replaces:
        # the draws are kept (they move the generator), the modules are not.
        self._init_token_tables(train_data, d, normalize, init_std)
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
        self._init_state(dropout, entity_dropout, relation_dropout, seed)

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

    @staticmethod
    def _precompute_chunk():
        return PRECOMPUTE_CHUNK                        # (this module's: a test shrinks it)

    # -- AddLossModule / autograd bridge (the reference Trainer's path: trainer.py:142, 206-234) ---------------------
    def _train_slots(self, share=True):
        """the two slots over the module's parameters; share (train_step()): conv weight and batch-norm parameters of the
        module become views of the slot's flat buffer (one optimizer segment; a step on the slot moves the module)"""
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
        st = self._cached_autograd_step(loss, label_smoothing, lambda: self._train_slots(share=False))
        for sl, relation in ((st.entity, False), (st.relation, True)):
            emb, tok, conv, bn = self._parts(relation)
            sl.conv.copy_(conv.weight.data)                                    # the module's parameters may have been stepped outside
            if bn is not None:
                sl.running_mean, sl.running_var, sl.num_batches_tracked = bn.running_mean, bn.running_var, bn.num_batches_tracked
        return self._refresh_autograd_step(st)

    def autograd_params_and_grads(self, st):
        params, grads = [], []
        for sl, relation in ((st.entity, False), (st.relation, True)):
            params += self._params(relation)
            grads += [sl.dW, sl.d_conv] + ([sl.d_bn[:sl.d], sl.d_bn[sl.d:]] if sl.bn is not None else [])
        return params, grads

    def _state_segments(self, sl, relation):
        """optimizer_params_and_state: the token table, then the slot's flat buffer [conv | bn weight | bn bias]"""
        emb, tok, conv, bn = self._parts(relation)
        d, flat = sl.d, (sl.flat, sl.sum_flat)
        out = [(emb.weight, (sl.W, sl.sumW), 0), (conv.weight, flat, 0)]
        if bn is not None:
            out += [(bn.weight, flat, 2 * d * d), (bn.bias, flat, 2 * d * d + d)]
        return out


class BigramPoolingComplexRelationModel(ComplexRelationScorer, BigramPoolingRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


class BigramPoolingDistmultRelationModel(DistmultRelationScorer, BigramPoolingRelationEmbedder):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)


# registered like the reference's (model.py:1052-1066): getattr(Models, args["model"])
Models.BigramPoolingComplexRelationModel = BigramPoolingComplexRelationModel
Models.BigramPoolingDistmultRelationModel = BigramPoolingDistmultRelationModel
