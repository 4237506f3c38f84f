"""TokenBasedRelationEmbedder (openkge/model.py:561-712): what the embedders whose rows are computed from tokens share --
the unigram pooling (token_pooled.py) and, through token_encoder.TokenEncoderEmbedder, the LSTM (lstm.py) and the bigram
pooling (bigram.py): constructor pieces, the evaluation surface over the tables precomputed from tokens, the scaffolding of
the two training bridges (train_step(): a fused step with its own optimizer; autograd_step(): the cached step behind
trainer.AddLossModule).  A subclass brings _encode(ids, relation, stream), precompute_embeddings_from_tokens(), _parts,
_train_step_class, _train_slots() -> the two slots a fused step runs on, _state_segments, autograd_step and
autograd_params_and_grads.
"""
from __future__ import annotations

import torch

from . import hotpath as H
from . import virtual_tables as VT
from .model import RelationEmbedder
from .step_optim import state_views

BN_EPS, BN_MOMENTUM = 1e-5, 0.1                     # torch.nn.BatchNorm1d(momentum=0.1, eps=1e-5), model.py:611-612


def token_id_matrix(id_to_tokens_map, max_len, device="cpu"):
    """TokenBasedRelationEmbedder.__init__ (model.py:579-597): row i = the LAST max_len tokens of item i,
    right-padded with 0."""
    out = torch.zeros((len(id_to_tokens_map), max_len), dtype=torch.int32)
    for i, seq in enumerate(id_to_tokens_map):
        tail = list(seq)[-max_len:]
        out[i, :len(tail)] = torch.tensor(tail, dtype=torch.int32)
    return out.to(device)


def _flush_before_state_dict(module, prefix, keep_vars):
    module.flush_steps()


class TokenBasedRelationEmbedder(RelationEmbedder):
    what = None                        # "token-pooled" / "LSTM" / "bigram", for messages
    max_slot = None                    # the largest slot size the family's kernels take (None: no limit of its own)
    step_copies_batchnorm = True       # the step's slots hold COPIES of the batch-norm parameters (train_step keeps them in step)

    # -- constructor pieces --------------------------------------------------------------------------------------------
    def _refuse_unsupported(self, entity_slot_size, relation_slot_size, activation, project_relation, sparse):
        """the options no token embedder implements; -> the relation slot size"""
        if relation_slot_size is None or relation_slot_size <= 0:
            relation_slot_size = entity_slot_size
        if activation is not None:             # (the LSTM reference applies a module class to a tensor, model.py:976-977)
            raise NotImplementedError(f"activation / encoder_activiation is not implemented for the {self.what} embedder")
        if project_relation:
            raise NotImplementedError(f"project_relation is not implemented for the {self.what} embedder")
        if sparse:
            raise NotImplementedError(f"sparse gradients are not implemented for the {self.what} embedder")
        if relation_slot_size != entity_slot_size:
            raise NotImplementedError("unequal slot sizes: the relation slot size must equal the entity slot size")
        if self.max_slot is not None and entity_slot_size > self.max_slot:
            raise NotImplementedError(f"{self.what} slot sizes above {self.max_slot}")
        return relation_slot_size

    @staticmethod
    def _max_lengths(train_data):
        max_len = train_data.max_length
        return (max_len, max_len) if isinstance(max_len, int) else (max_len[0], max_len[1])

    def _init_token_tables(self, train_data, d, normalize, init_std):
        """The reference's constructor order (TokenBasedRelationEmbedder.__init__, model.py:568-634): token-id matrices,
        embeddings, batch-norm modules with uniform_ weights, then the embeddings' normal_ -- the same torch.manual_seed
        gives bit-identical initial parameters."""
        e_len, r_len = self._max_lengths(train_data)
        self.train_data, self.slot_size, self.relation_slot_size, self.normalize = train_data, d, d, normalize
        self.register_buffer('entity_token_ids', token_id_matrix(train_data.entity_id_to_tokens_map, e_len))
        self.register_buffer('relation_token_ids', token_id_matrix(train_data.relation_id_to_tokens_map, r_len))
        self.entity_embedding = torch.nn.Embedding(train_data.entity_tokens_size, d, padding_idx=0)
        self.relation_embedding = torch.nn.Embedding(train_data.relation_tokens_size, d, padding_idx=0)
        self.entity_batchnorm = self.relation_batchnorm = None
        if normalize == 'batchnorm':
            self.entity_batchnorm = torch.nn.BatchNorm1d(d, momentum=BN_MOMENTUM, eps=BN_EPS)
            self.relation_batchnorm = torch.nn.BatchNorm1d(d, momentum=BN_MOMENTUM, eps=BN_EPS)
            torch.nn.init.uniform_(self.entity_batchnorm.weight)
            torch.nn.init.uniform_(self.relation_batchnorm.weight)
        torch.nn.init.normal_(self.entity_embedding.weight.data, std=init_std)          # row 0 included
        torch.nn.init.normal_(self.relation_embedding.weight.data, std=init_std)

    def _init_state(self, dropout, entity_dropout, relation_dropout, seed):
        """after the encoder modules: dropout fall-backs (model.py:757-758, :845-846, :953-954) and the embedder's own state"""
        self.entity_dropout = entity_dropout if entity_dropout else dropout
        self.relation_dropout = relation_dropout if relation_dropout else dropout
        self.entity_projection = self.relation_projection = None                       # the attribute model.py:789 reads
        self.entity_embedding_from_tokens = self.relations_embedding_from_tokens = None
        self.dropout_seed, self.dropout_step = seed, 0
        self._engine = None
        # training drivers that update this module's parameters in place and may owe deferred updates (weak references, see
        # the token-pooled train_step()): every reader of the parameters settles them first
        self._steps = []
        self.register_state_dict_pre_hook(_flush_before_state_dict)

    def __getstate__(self):                              # (weak references do not pickle; a copy starts without drivers)
        state = self.__dict__.copy()
        state["_steps"] = []
        return state

    def flush_steps(self):
        for ref in self._steps:
            st = ref()
            if st is not None:
                st.flush()

    # -- plumbing ------------------------------------------------------------------------------------------------------
    def engine(self):
        dev = self.entity_embedding.weight.device
        if self._engine is None or self._engine.device != dev:
            self._engine = H.HotPath(dev)
        return self._engine

    def _parts(self, relation):
        """-> (embedding, token-id matrix, encoder module or None, batch-norm or None) of one slot"""
        if relation:
            return self.relation_embedding, self.relation_token_ids, None, self.relation_batchnorm
        return self.entity_embedding, self.entity_token_ids, None, self.entity_batchnorm

    def encode_subj(self, subj):
        return self._encode(subj, False, H.STREAM_SP_ENT)

    def encode_obj(self, obj):
        return self._encode(obj, False, H.STREAM_PO_ENT)

    def encode_rel(self, rel):
        return self._encode(rel, True, H.STREAM_SP_REL)

    # -- tables precomputed from tokens (model.py:624-712) ---------------------------------------------------------------
    def train(self, mode=True):
        self.entity_embedding_from_tokens = self.relations_embedding_from_tokens = None
        return super().train(mode)

    def get_all_subj(self):
        self.precompute_embeddings_from_tokens()
        return self.entity_embedding_from_tokens[self.train_data.min_entities_size:]

    get_all_obj = get_all_subj

    def get_all_rel(self):
        self.precompute_embeddings_from_tokens()
        return self.relations_embedding_from_tokens[self.train_data.min_entities_size:]        # sic, model.py:630

    def get_subj(self, subj):
        self.precompute_embeddings_from_tokens()
        return self.entity_embedding_from_tokens[subj].unsqueeze(0)

    get_obj = get_subj

    def get_rel(self, rel):
        self.precompute_embeddings_from_tokens()
        return self.relations_embedding_from_tokens[rel]

    def get_slot_size(self):
        return self.slot_size

    # -- prefix scoring: RelationScorer.sp_prefix_score / po_prefix_score (model.py:52-74) ------------------------------
    def _prefix_score(self, batch: H.PrefixBatch, many=None):
        if many is None:
            many = self.get_all_obj()
        if batch.sp_subj is not None:
            return self._score(self.encode_subj(batch.sp_subj), self.encode_rel(batch.sp_rel), many, prefix=True, sp=True, po=False)
        return self._score(many, self.encode_rel(batch.po_rel), self.encode_obj(batch.po_obj), prefix=True, sp=False, po=True)

    # -- top-k prediction over the tables precomputed from tokens (RelationScorer.sp_prefix_topk / po_prefix_topk) -------
    def _any_dropout(self):
        return max(self.entity_dropout or 0.0, self.relation_dropout or 0.0) > 0

    def _prefix_topk(self, batch: H.PrefixBatch, k, filt_ptr, filt_col):
        self.precompute_embeddings_from_tokens()
        E, R = self.entity_embedding_from_tokens, self.relations_embedding_from_tokens
        if batch.cand_ids is None:
            batch.cand_first = self.train_data.min_entities_size
            batch.n_cand = E.shape[0] - batch.cand_first
        scores, cols, ids = self.engine().topk_prefixes(E.contiguous(), R.contiguous(), self.scorer_name, batch, k, filt_ptr, filt_col)
        return scores, ids, cols

    def loss_only(self, batch: H.PrefixBatch, loss, label_smoothing, scores=None):
        """eval-mode loss (+ scores) of AddLossModule: rows encoded with the running statistics, no dropout"""
        eng, dev = self.engine(), self.entity_embedding.weight.device
        n_po, n_sp, n_c = batch.n_po, batch.n_sp, batch.n_candidates
        if batch.cand_ids is None:
            cand = self.get_all_obj()[batch.cand_first - self.train_data.min_entities_size:][:n_c] if not self.training else \
                self._encode(torch.arange(batch.cand_first, batch.cand_first + n_c, dtype=torch.int32, device=dev), False, H.STREAM_CAND).squeeze(1)
        else:
            cand = self._encode(batch.cand_ids, False, H.STREAM_CAND).squeeze(1)
        parts_e, parts_r = [cand], []
        if n_po:
            parts_r.append(self.encode_rel(batch.po_rel).squeeze(1))
            parts_e.append(self.encode_obj(batch.po_obj).squeeze(1))
        if n_sp:
            parts_e.append(self.encode_subj(batch.sp_subj).squeeze(1))
            parts_r.append(self.encode_rel(batch.sp_rel).squeeze(1))
        EV, RV = torch.cat(parts_e).contiguous(), torch.cat(parts_r).contiguous()
        vb = VT.VirtualTables(dev).batch(n_c, n_po, n_sp, batch.pos_row, batch.pos_col)
        return eng.forward_backward(EV, RV, self.scorer_name, vb, None, None, loss=loss, label_smoothing=label_smoothing,
                                    normalizer=1.0, scores=scores, loss_only=True)

    # -- the training bridges ----------------------------------------------------------------------------------------------
    def _build_step(self, slots, **kw):
        return self._train_step_class(slots[0], slots[1], self.scorer_name, dropout=self.entity_dropout,
                                      relation_dropout=self.relation_dropout, seed=self.dropout_seed, **kw)

    def train_step(self, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8, label_smoothing=0.0, optimizer="adagrad", betas=(0.9, 0.999),
                   grad_clip=0.0):
        """The training driver for this model: shares the module's parameters (updated in place; what _train_slots() does
        to them for that is the subclass's).  optimizer / betas / grad_clip: as on FusedTrainStep."""
        st = self._build_step(self._train_slots(), loss=loss, lr=lr, weight_decay=weight_decay, eps=eps, label_smoothing=label_smoothing,
                              optimizer=optimizer, betas=betas, grad_clip=grad_clip)
        if self.step_copies_batchnorm and self.entity_batchnorm is not None:
            st.module_batchnorms = ((st.entity, self.entity_batchnorm), (st.relation, self.relation_batchnorm))
        return st

    def _cached_autograd_step(self, loss, label_smoothing, make_slots, **kw):
        """the cached train step behind AddLossModule (trainer.py:142, 206-234): rebuilt when the loss, the smoothing or the
        module's tables changed; its optimizer is NOT used (the caller's torch optimizer steps the module parameters)"""
        st = getattr(self, "_ag_step", None)
        if st is None or st.loss != loss or st.label_smoothing != label_smoothing or \
                st.entity.W.data_ptr() != self.entity_embedding.weight.data_ptr():
            st = self._ag_step = self._build_step(make_slots(), loss=loss, label_smoothing=label_smoothing, **kw)
        return st

    def _refresh_autograd_step(self, st):
        """every autograd_step() call, after the subclass has pointed the slots at its encoder tensors: fresh gradient buffers
        (the last ones went to autograd), the module's batch-norm parameters (they may have been stepped outside) in the slots'
        copies, and this call's dropout step"""
        for sl, relation in ((st.entity, False), (st.relation, True)):
            bn = self._parts(relation)[3]
            sl.dW = torch.zeros_like(sl.W)
            if bn is not None:
                sl.bn[:sl.d].copy_(bn.weight.data)
                sl.bn[sl.d:].copy_(bn.bias.data)
            sl.fresh_grads()
        st.steps = self.dropout_step
        self.dropout_step += 1
        return st

    def optimizer_params_and_state(self, st):
        """For checkpoint.py, `st` = the driver train_step() returned: ([(parameter, views of the step's optimizer state that
        belong to it -- (sum,) under Adagrad, (exp_avg, exp_avg_sq) under Adam, each of the parameter's shape --, whether the step
        moves it), ...] in self.parameters() order, the Adam device state word or None).  The subclass says in
        _state_segments(slot, relation) which part of which flat buffer is whose; a slot the scorer leaves unused (bias_entity)
        is listed as not moved."""
        found = {}
        for sl, relation in ((st.entity, False), (st.relation, True)):
            moved = not st._unused(sl)
            for p, (buf, acc), offset in self._state_segments(sl, relation):
                found[p] = (state_views(st.optimizer_state_of(buf, acc), offset, p), moved)
        return [(p,) + found[p] for p in self.parameters()], st.adam_word()
