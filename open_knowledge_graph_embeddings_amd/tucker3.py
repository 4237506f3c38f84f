"""Tucker3 lookup model: RescalRelationScorer + LookupBaseRelationEmbedder with project_relation (openkge/model.py:142-173,
:353-542, :1001-1004) over the HIP kernels of csrc/okge_tucker3.hip.

    M_b = reshape(W rho_b, (d, d))        W = relation_projection.0.weight (d^2, r_e), rho = rows of the (|R|, r_e) relation table
    sp:  q_b = e_b^T M_b      po:  q_b = M_b e_b      scores[b, :] = q_b . Cand^T

Everything from q on is the tile kernels' work on a caller-supplied query block (HotPath.train_tiles / okge_score_queries /
okge_row_logsumexp / okge_evaluate_fused_shard; the tables descriptor they get names the ENTITY table twice -- the relation slot
of the descriptor is never dereferenced by these calls -- and the DistMult scorer id, which they do not look at).  In front of
them: okge_encode_rows (masked prefix rows) -> okge_tucker3_fold; behind them: okge_tucker3_backward -> okge_scatter_rows.
M (B, d^2) is never materialised on the training path.
"""
from __future__ import annotations

import torch

from . import _native as N
from . import hotpath as H
from .step_optim import StepOptimizer, check_optimizer
from .model import LookupBaseRelationEmbedder, Models, PAD, RelationEmbedder, RelationScorer, _wants_grad

MAX_SLOT = 256                                     # d and r_e the fold / backward kernels take
TILE_SCORER = "distmult"                           # (not looked at by the query-block calls; DistMult has no even-d rule)


class Tucker3Kernels:
    """ctypes driver of okge_tucker3_* for one device, with its own workspace."""

    def __init__(self, engine: H.HotPath):
        self.engine, self.lib, self.device = engine, engine.lib, engine.device
        self.ws, self.ws_bytes = None, 0

    def _workspace(self, rows, d, r):
        need = int(self.lib.okge_tucker3_workspace_bytes(rows, d, r))
        if need == 0:
            raise N.OkgeError(f"tucker3: unsupported size rows={rows} d={d} r_e={r} (1 <= d, r_e <= {MAX_SLOT})")
        if need > self.ws_bytes:
            self.ws = None
            self.ws, self.ws_bytes = torch.empty(need, dtype=torch.uint8, device=self.device), need
        return self.ws

    def fold(self, W, ent_rows, rel_rows, n_po, n_sp, Q=None):
        """-> the query block [okge_query_rows(B)][okge_query_ld(d)] of the masked prefix rows (po rows first)"""
        d, r = ent_rows.shape[1], rel_rows.shape[1]
        B = n_po + n_sp
        rows, ld = self.engine.query_shape(B, d)
        if Q is None:
            Q = torch.empty((rows, ld), dtype=torch.float32, device=self.device)
        ws = self._workspace(B, d, r)
        N.check(self.lib.okge_tucker3_fold(W.data_ptr(), d, r, ent_rows.data_ptr(), ent_rows.stride(0), rel_rows.data_ptr(),
                                           rel_rows.stride(0), n_po, n_sp, Q.data_ptr(), Q.stride(0), ws.data_ptr(), self.ws_bytes,
                                           self.engine._stream()), "okge_tucker3_fold")
        return Q

    def backward(self, W, ent_rows, rel_rows, dQ, n_po, n_sp, d_ent=None, d_rel=None, dW=None, fresh=True):
        d, r = ent_rows.shape[1], rel_rows.shape[1]
        ws = self._workspace(n_po + n_sp, d, r)
        N.check(self.lib.okge_tucker3_backward(W.data_ptr(), d, r, ent_rows.data_ptr(), ent_rows.stride(0), rel_rows.data_ptr(),
                                               rel_rows.stride(0), dQ.data_ptr(), dQ.stride(0), n_po, n_sp,
                                               N.OKGE_TRAIN_GRADS_ZERO if fresh else 0, H._ptr(d_ent), H._ptr(d_rel), H._ptr(dW),
                                               ws.data_ptr(), self.ws_bytes, self.engine._stream()), "okge_tucker3_backward")

    def score_triples(self, W, subj, rel, obj):
        """(b, 1) scores s^T M o of encoded rows subj / obj (b, d), rel (b, r_e)"""
        n, d, r = subj.shape[0], subj.shape[1], rel.shape[1]
        out = torch.empty((n, 1), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        ws = self._workspace(n, d, r)
        N.check(self.lib.okge_tucker3_score_triples(W.data_ptr(), d, r, subj.data_ptr(), subj.stride(0), rel.data_ptr(), rel.stride(0),
                                                    obj.data_ptr(), obj.stride(0), n, out.data_ptr(), ws.data_ptr(), self.ws_bytes,
                                                    self.engine._stream()), "okge_tucker3_score_triples")
        return out


    def apply(self, M, x, transpose):
        """x^T M (transpose False) / M x (True) per row on materialised (n, d^2) matrices"""
        n, d = x.shape
        out = torch.empty((n, d), dtype=torch.float32, device=self.device)
        N.check(self.lib.okge_tucker3_apply(M.data_ptr(), M.stride(0), x.data_ptr(), x.stride(0), n, d, 1 if transpose else 0, out.data_ptr(),
                                            out.stride(0), self.engine._stream()), "okge_tucker3_apply")
        return out

    def outer(self, u, v):
        """(n, d^2) rows u_b (x) v_b"""
        n, d = u.shape
        out = torch.empty((n, d * d), dtype=torch.float32, device=self.device)
        N.check(self.lib.okge_tucker3_outer(u.data_ptr(), u.stride(0), v.data_ptr(), v.stride(0), n, d, out.data_ptr(), out.stride(0),
                                            self.engine._stream()), "okge_tucker3_outer")
        return out


class Tucker3TrainStep(StepOptimizer):
    """forward + loss + backward + Adagrad for LookupTucker3RelationModel (Trainer.compute_one_batch, trainer.py:181-257):
    encode rows -> fold -> train tiles -> tucker3 backward -> scatter -> one dense Adagrad launch over (E, R, W).
    E (|E|, d), R (|R|, r_e), W (d^2, r_e) are updated in place.  dropout = the entity rows' and candidates' drop probability
    (input_dropout and dropout combined), relation_dropout = the relation rows' (relation_input_dropout).  optimizer / betas /
    grad_clip: as on FusedTrainStep (step_optim.py), over E, R and W."""

    def __init__(self, E, R, W, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8, label_smoothing=0.0, dropout=0.0,
                 relation_dropout=0.0, seed=0, engine=None, optimizer="adagrad", betas=(0.9, 0.999), grad_clip=0.0):
        check_optimizer(optimizer, betas)
        for t in (E, R, W):
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise N.OkgeError("tucker3: parameters must be contiguous fp32 tensors")
        d, r = E.shape[1], R.shape[1]
        if W.shape != (d * d, r):
            raise N.OkgeError(f"tucker3: the projection must be (d^2, r_e) = ({d * d}, {r}), got {tuple(W.shape)}")
        if not (1 <= d <= MAX_SLOT and 1 <= r <= MAX_SLOT):
            raise NotImplementedError(f"tucker3: slot / relation sizes above {MAX_SLOT}")
        self.E, self.R, self.W, self.loss = E, R, W, loss
        self.d, self.r = d, r
        self.lr, self.weight_decay, self.eps, self.label_smoothing = lr, weight_decay, eps, label_smoothing
        self.dropout, self.relation_dropout, self.seed, self.steps = dropout, relation_dropout, seed, 0
        self.device = E.device
        self.engine = engine or H.HotPath(self.device)
        self.kernels = Tucker3Kernels(self.engine)
        self.dE, self.dR, self.dW = torch.zeros_like(E), torch.zeros_like(R), torch.zeros_like(W)
        self.sumE, self.sumR, self.sumW = torch.zeros_like(E), torch.zeros_like(R), torch.zeros_like(W)
        self.loss_out = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.shard = H.Shard(0, E.shape[0], 0)
        self._B = -1
        self._init_optimizer(optimizer, betas, grad_clip)

    def state_tensors(self):
        return [self.E, self.R, self.W, self.dE, self.dR, self.dW, self.sumE, self.sumR, self.sumW] + self._optimizer_state()

    def _param_groups(self, every=False):
        return [(self.E, self.dE, self.sumE), (self.R, self.dR, self.sumR), (self.W, self.dW, self.sumW)]

    def flush(self):
        """(no deferred updates here: every parameter is current after every step)"""

    # -- pieces ------------------------------------------------------------------------------------------------------
    def _buffers(self, B):
        if B != self._B:
            dev = self.device
            rows, ld = self.engine.query_shape(B, self.d)
            self._B = B
            self.ent_rows = torch.empty((B, self.d), device=dev)
            self.rel_rows = torch.empty((B, self.r), device=dev)
            self.Q, self.dQ = torch.empty((rows, ld), device=dev), torch.empty((rows, ld), device=dev)
            self.d_ent, self.d_rel = torch.empty((B, self.d), device=dev), torch.empty((B, self.r), device=dev)

    def _drops(self, batch, training=True):
        """the five masks of a step; a batch that brings explicit specs (captured keep-masks) keeps them"""
        given = (batch.drop_cand, batch.drop_po_ent, batch.drop_po_rel, batch.drop_sp_ent, batch.drop_sp_rel)
        if any(g.p > 0 for g in given) or not training:
            return given if training else (H.NO_DROP,) * 5
        return H.dropout_specs(self.dropout, self.relation_dropout, self.seed, self.steps)

    def encode_and_fold(self, batch, drops):
        """masked prefix rows of the batch (okge_encode_rows, per direction: each has its own mask stream) -> query block"""
        eng, dev = self.engine, self.device
        n_po, n_sp = batch.n_po, batch.n_sp
        self._buffers(n_po + n_sp)
        _, d_po_e, d_po_r, d_sp_e, d_sp_r = drops
        if n_po:
            eng.encode_rows(self.E, H._i32(batch.po_obj, dev), drop=d_po_e, out=self.ent_rows[:n_po])
            eng.encode_rows(self.R, H._i32(batch.po_rel, dev), drop=d_po_r, out=self.rel_rows[:n_po])
        if n_sp:
            eng.encode_rows(self.E, H._i32(batch.sp_subj, dev), drop=d_sp_e, out=self.ent_rows[n_po:])
            eng.encode_rows(self.R, H._i32(batch.sp_rel, dev), drop=d_sp_r, out=self.rel_rows[n_po:])
        return self.kernels.fold(self.W, self.ent_rows, self.rel_rows, n_po, n_sp, self.Q)

    def _cand_batch(self, batch, drop_cand):
        return H.PrefixBatch(pos_row=batch.pos_row, pos_col=batch.pos_col, cand_ids=batch.cand_ids, cand_first=batch.cand_first,
                             n_cand=batch.n_cand, cand_unique=batch.cand_unique, drop_cand=drop_cand)

    def _tiles(self, cb, B, normalizer, loss_only, grads_zero=True):
        """the tile kernels on the folded queries (HotPath.train_tiles): loss, candidate gradients into dE, dQ"""
        eng, E = self.engine, self.E
        row_lse = None
        if self.loss == "kl":
            row_lse = eng.row_logsumexp(E, E, TILE_SCORER, self.Q, B, cb, self.shard)
        return eng.train_tiles(E, E, TILE_SCORER, self.Q, cb, self.shard, self.dE, self.dQ, cb.n_candidates, loss=self.loss,
                               label_smoothing=self.label_smoothing if self.loss == "bce" else 0.0, normalizer=normalizer,
                               loss_out=self.loss_out, grads_zero=grads_zero, row_lse=row_lse, loss_only=loss_only, B=B)

    # -- the step --------------------------------------------------------------------------------------------------------
    def step(self, batch: H.PrefixBatch, normalizer=None):
        loss = self.forward_backward(batch, normalizer)
        self.optimizer_step()
        return loss

    def forward_backward(self, batch: H.PrefixBatch, normalizer=None, scores=None, accumulate=False):
        """Leaves the dense gradients in dE, dR, dW; returns the summed loss as a device double[1].  accumulate=False: the three
        buffers are zero on entry (optimizer_step clears them), candidate rows and dW are stored; accumulate=True: all three are
        added to (a second batch before the optimizer step).  scores: optional (B, N) buffer for all_outputs."""
        self.steps += 1
        eng, dev = self.engine, self.device
        n_po, n_sp = batch.n_po, batch.n_sp
        B = n_po + n_sp
        drops = self._drops(batch)
        self.encode_and_fold(batch, drops)
        cb = self._cand_batch(batch, drops[0])
        if scores is not None:
            eng.score_queries(self.E, self.E, TILE_SCORER, self.Q, B, cb, self.shard, out=scores)
        self._tiles(cb, B, normalizer, loss_only=False, grads_zero=not accumulate)
        self.kernels.backward(self.W, self.ent_rows, self.rel_rows, self.dQ, n_po, n_sp, self.d_ent, self.d_rel, self.dW, fresh=not accumulate)
        _, d_po_e, d_po_r, d_sp_e, d_sp_r = drops
        if n_po:
            eng.scatter_rows(self.d_ent[:n_po], H._i32(batch.po_obj, dev), 0, self.dE, d_po_e)
            eng.scatter_rows(self.d_rel[:n_po], H._i32(batch.po_rel, dev), 0, self.dR, d_po_r)
        if n_sp:
            eng.scatter_rows(self.d_ent[n_po:], H._i32(batch.sp_subj, dev), 0, self.dE, d_sp_e)
            eng.scatter_rows(self.d_rel[n_po:], H._i32(batch.sp_rel, dev), 0, self.dR, d_sp_r)
        return self.loss_out

    def loss_only(self, batch: H.PrefixBatch, scores=None, normalizer=1.0):
        """forward + summed loss without gradients or dropout (validation loss, trainer.py:363-369)"""
        B = batch.B
        drops = self._drops(batch, training=False)
        self.encode_and_fold(batch, drops)
        cb = self._cand_batch(batch, H.NO_DROP)
        if scores is not None:
            self.engine.score_queries(self.E, self.E, TILE_SCORER, self.Q, B, cb, self.shard, out=scores)
        return self._tiles(cb, B, normalizer, loss_only=True)

    def optimizer_step(self):
        self._update(self._param_groups())

    # -- evaluation ------------------------------------------------------------------------------------------------------
    def scores(self, batch: H.PrefixBatch, out=None):
        """(B, N) eval-mode scores of the batch's prefixes against its candidates (materialised: okge_score_queries)"""
        self.encode_and_fold(batch, (H.NO_DROP,) * 5)
        return self.engine.score_queries(self.E, self.E, TILE_SCORER, self.Q, batch.B, self._cand_batch(batch, H.NO_DROP), self.shard, out=out)

    def ranks(self, batch: H.PrefixBatch, filt_ptr, filt_col, row_ptr, grp_ptr, ids):
        """filtered ranks (int64 per answer group; dataset.py:423-446) through the fused evaluator fed with the folded query
        block, as a one-rank shard: no (B, N) score tensor"""
        eng, dev = self.engine, self.device
        n_groups = int(grp_ptr.numel()) - 1
        counts = torch.zeros((max(n_groups, 1), 2), dtype=torch.int64, device=dev)
        if n_groups == 0:
            return counts[:0, 0]
        self.encode_and_fold(batch, (H.NO_DROP,) * 5)
        true = torch.full((n_groups,), float("-inf"), dtype=torch.float32, device=dev)
        cb = self._cand_batch(batch, H.NO_DROP)
        args = (self.E, self.E, TILE_SCORER, self.Q, batch.B, cb, self.shard, cb.n_candidates, filt_ptr, filt_col, row_ptr, grp_ptr, ids,
                true, counts)
        for phase in (1, 2, 4):
            eng.evaluate_fused_shard(phase, *args)
        return counts[:n_groups, 0] + counts[:n_groups, 1] // 2


class Tucker3PrefixScoreFn(torch.autograd.Function):
    """sp_prefix_score / po_prefix_score with gradients enabled (a caller's own loss on the (b, N) scores): forward = masked rows
    -> fold -> okge_score_queries on encoded candidate rows; backward = dQ = g . cand and d_cand = g^T . Q on the fp32 MFMA product
    of okge_prefix_score_backward (called with the query rows as DistMult entity rows against all-one relation rows: its fold is
    then the identity), then okge_tucker3_backward.  Inputs: the encoded rows, so that autograd carries their gradients on through
    EncodeRowsFn into the tables; W directly."""

    @staticmethod
    def forward(ctx, ent, rel, cand, W, kernels, sp):
        ent_c, rel_c, cand_c, W_c = ent.detach().contiguous(), rel.detach().contiguous(), cand.detach().contiguous(), W.detach()
        b = ent_c.shape[0]
        n_po, n_sp = (0, b) if sp else (b, 0)
        eng = kernels.engine
        Q = kernels.fold(W_c, ent_c, rel_c, n_po, n_sp)
        cb = H.PrefixBatch(cand_first=0, n_cand=cand_c.shape[0])
        ctx.save_for_backward(ent_c, rel_c, cand_c, W_c, Q)
        ctx.kernels, ctx.split = kernels, (n_po, n_sp)
        return eng.score_queries(cand_c, cand_c, TILE_SCORER, Q, b, cb, H.Shard(0, cand_c.shape[0], 0))

    @staticmethod
    def backward(ctx, g):
        ent, rel, cand, W, Q = ctx.saved_tensors
        k, eng = ctx.kernels, ctx.kernels.engine
        n_po, n_sp = ctx.split
        b, d = ent.shape
        g = g.contiguous()
        need_e, need_r, need_c, need_w = ctx.needs_input_grad[:4]
        ones = torch.ones((b, d), dtype=torch.float32, device=g.device)
        dQ, _, d_cand = eng.prefix_score_backward(TILE_SCORER, True, g, Q[:b, :d], ones, cand, True, False, need_c)
        d_ent = torch.empty_like(ent) if need_e else None
        d_rel = torch.empty_like(rel) if need_r else None
        dW = torch.empty_like(W) if need_w else None
        k.backward(W, ent, rel, dQ, n_po, n_sp, d_ent, d_rel, dW, fresh=True)
        return d_ent, d_rel, d_cand, dW, None, None


# ------------------------------------------------------------------------------------------------------------------
# API-compatible model classes
# ------------------------------------------------------------------------------------------------------------------
class ProjectRelFn(torch.autograd.Function):
    """encode_rel's Linear (model.py:402-408): (b, r_e) relation rows -> (b, d^2) projected rows = rows . W^T.  Off the training path
    (which never forms these rows): the product is okge_score_queries with W as the candidate table and the rows as queries;
    backward d_rows = g . W, dW = g^T . rows on okge_prefix_score_backward (DistMult fold against all-one relation rows = identity)"""

    @staticmethod
    def forward(ctx, rows, W, kernels):
        rows_c, W_c = rows.detach().contiguous(), W.detach()
        eng = kernels.engine
        b, r = rows_c.shape
        n_rows, ld = eng.query_shape(max(b, 1), r)
        Q = torch.zeros((n_rows, ld), dtype=torch.float32, device=rows_c.device)
        Q[:b, :r] = rows_c
        ctx.save_for_backward(rows_c, W_c)
        ctx.kernels = kernels
        if b == 0:
            return torch.empty((0, W_c.shape[0]), dtype=torch.float32, device=rows_c.device)
        cb = H.PrefixBatch(cand_first=0, n_cand=W_c.shape[0])
        return eng.score_queries(W_c, W_c, TILE_SCORER, Q, b, cb, H.Shard(0, W_c.shape[0], 0)).contiguous()

    @staticmethod
    def backward(ctx, g):
        rows, W = ctx.saved_tensors
        need_r, need_w = ctx.needs_input_grad[:2]
        ones = torch.ones_like(rows)
        d_rows, _, dW = ctx.kernels.engine.prefix_score_backward(TILE_SCORER, True, g.contiguous(), rows, ones, W, need_r, False, need_w)
        return d_rows, dW, None


class ApplyRelFn(torch.autograd.Function):
    """x^T M (transpose = False: subj.bmm(rel)) or M x (True: rel.bmm(obj)) on MATERIALISED relation matrices M (b, d^2)
    (model.py:160-171): okge_tucker3_apply; backward the transposed product and the outer-product gradient of M"""

    @staticmethod
    def forward(ctx, M, x, transpose, kernels):
        M_c, x_c = M.detach().contiguous(), x.detach().contiguous()
        ctx.save_for_backward(M_c, x_c)
        ctx.kernels, ctx.transpose = kernels, bool(transpose)
        return kernels.apply(M_c, x_c, transpose)

    @staticmethod
    def backward(ctx, g):
        M, x = ctx.saved_tensors
        k, g = ctx.kernels, g.contiguous()
        dM = dx = None
        if ctx.needs_input_grad[0]:
            dM = k.outer(g, x) if ctx.transpose else k.outer(x, g)
        if ctx.needs_input_grad[1]:
            dx = k.apply(M, g, not ctx.transpose)
        return dM, dx, None, None


class Tucker3TripleFn(torch.autograd.Function):
    """forward(subj, rel, obj) on ids with gradients enabled: score_b = s_b . (M_b o_b) through okge_tucker3_score_triples without
    forming M; backward d_subj = g (M o) (the po fold again), and dq = g s through okge_tucker3_backward for d_obj, d_rel, dW"""

    @staticmethod
    def forward(ctx, subj, rel, obj, W, kernels):
        s, r, o, W_c = subj.detach().contiguous(), rel.detach().contiguous(), obj.detach().contiguous(), W.detach()
        ctx.save_for_backward(s, r, o, W_c)
        ctx.kernels = kernels
        return kernels.score_triples(W_c, s, r, o)

    @staticmethod
    def backward(ctx, g):
        s, r, o, W = ctx.saved_tensors
        k = ctx.kernels
        b, d = s.shape
        g = g.reshape(b, 1).contiguous()
        Q = k.fold(W, o, r, b, 0)
        d_s = g * Q[:b, :d] if ctx.needs_input_grad[0] else None
        dQ = torch.zeros_like(Q)
        dQ[:b, :d] = g * s
        d_o = torch.empty_like(o) if ctx.needs_input_grad[2] else None
        d_r = torch.empty_like(r) if ctx.needs_input_grad[1] else None
        dW = torch.empty_like(W) if ctx.needs_input_grad[3] else None
        k.backward(W, o, r, dQ, b, 0, d_o, d_r, dW, fresh=True)
        return d_s, d_r, d_o, dW, None


# ------------------------------------------------------------------------------------------------------------------
# API-compatible model classes
# ------------------------------------------------------------------------------------------------------------------
class RescalRelationScorer(RelationScorer):
    """openkge/model.py:142-173: score = s^T M o with M = the relation's (d, d) matrix.  triple_score / _score take ENCODED rows with
    the reference's shapes -- rel is the (b, d^2) block encode_rel returns -- and carry an autograd graph when their inputs do;
    forward (ids) and the prefix scores (ids) never form those rows."""
    scorer_name = "rescal"

    def forward(self, subj, rel, obj, **kwargs):
        """(b, 1) scores of id triples: triple_score(encode_subj, encode_rel, encode_obj) (model.py:36-41, :144-145) without the
        (b, d^2) rows; with gradients enabled the result carries a graph into the three parameters"""
        weight = self.relation_projection[0].weight
        s = self.encode_subj(subj).reshape(-1, self.slot_size)
        r = self._rel_rows(rel).reshape(-1, self.relation_size)
        o = self.encode_obj(obj).reshape(-1, self.slot_size)
        if _wants_grad(s, r, o, weight):
            return Tucker3TripleFn.apply(s, r, o, weight, self.kernels())
        return self.kernels().score_triples(self.W, s.detach().contiguous(), r.detach().contiguous(), o.detach().contiguous())

    def _rel_matrices(self, rel):
        d2 = self.slot_size ** 2
        if rel.shape[-1] != d2:
            raise ValueError(f"rel must be the (b, d^2) = (b, {d2}) rows encode_rel returns, got {tuple(rel.shape)}")
        return rel.reshape(-1, d2)

    def triple_score(self, subj, rel, obj, **kwargs):
        """subj.bmm(rel.bmm(obj)) on encoded rows: subj / obj (b, d), rel (b, d^2) (model.py:144-145, :167-171)"""
        from . import autograd_score as AG
        d = self.slot_size
        s, o, M = subj.reshape(-1, d), obj.reshape(-1, d), self._rel_matrices(rel)
        q = ApplyRelFn.apply(M, o, True, self.kernels())
        ones = torch.ones_like(q)
        if _wants_grad(s, q):
            return AG.triple_score("distmult", s, ones, q)
        return self.engine().score_triples("distmult", s.detach().contiguous(), ones, q.detach())

    def _score(self, subj, rel, obj, prefix=False, sp=None, po=None):
        """model.py:147-173 on ALREADY ENCODED rows: (b, d), (b, d^2), (N, d) -> (b, N), or the triple scores"""
        from . import autograd_score as AG
        if not prefix:
            return self.triple_score(subj, rel, obj)
        if not sp and not po:
            raise Exception      # model.py:165-166
        flat = lambda t: t.reshape(-1, t.shape[-1])      # noqa: E731
        ent, cand = (flat(subj), flat(obj)) if sp else (flat(obj), flat(subj))
        q = ApplyRelFn.apply(self._rel_matrices(rel), ent, not sp, self.kernels())
        # scores = q . cand^T: the DistMult prefix scorer against all-one relation rows
        return AG.PrefixScoreFn.apply(q, torch.ones_like(q), cand, self.engine(), "distmult", True)


class ProjectedLookupRelationEmbedder(LookupBaseRelationEmbedder):
    """LookupBaseRelationEmbedder with project_relation=True (openkge/model.py:353-542): the relation's d x d matrix is a Linear
    (no bias) of its r_e-sized embedding.  Implemented on the HIP path: input_dropout / dropout (entity rows and candidates),
    relation_input_dropout, relation_slot_size / relation_embedding_size != entity_slot_size, sizes up to 256.  Not implemented
    (raise at construction): relation_dropout > 0 (a mask over the d^2 projected entries), project_relation_activation,
    project_entity, batch_norm, normalize, l2_reg > 0, sparse, entity_embedding_size != entity_slot_size."""

    fused_step_model = True            # trainer.AddLossModule: the model brings its own fused step (autograd_step / loss_only)

    def __init__(self, entity_slot_size, relation_slot_size, train_data, entity_embedding_size=None, relation_embedding_size=None,
                 normalize='', dropout=0.0, input_dropout=0.0, relation_dropout=0.0, relation_input_dropout=0.0, project_entity=False,
                 project_entity_activation='ReLU', project_relation=True, project_relation_activation=None, sparse=False,
                 init_std=0.01, batch_norm=False, l2_reg=0, seed=0):
        RelationEmbedder.__init__(self)
        if relation_slot_size is None or relation_slot_size <= 0:
            relation_slot_size = entity_slot_size
        e_size = entity_slot_size if entity_embedding_size is None else entity_embedding_size
        r_size = relation_slot_size if relation_embedding_size is None else relation_embedding_size
        if not project_relation:
            raise NotImplementedError("the RESCAL scorer without the relation projection (a (|R|, d^2) table) is not implemented")
        if (dropout if relation_dropout is None else relation_dropout) > 0:
            raise NotImplementedError("relation_dropout > 0: a mask over the d^2 projected entries is not implemented")
        if project_relation_activation:
            raise NotImplementedError("project_relation_activation is not implemented")
        if project_entity:
            raise NotImplementedError("project_entity is not implemented for the Tucker3 model")
        if batch_norm:
            raise NotImplementedError("batch_norm is not implemented for the Tucker3 model")
        if normalize:
            raise NotImplementedError(f"normalize={normalize!r} is not implemented for the Tucker3 model")
        if l2_reg and l2_reg > 0:
            raise NotImplementedError("l2_reg > 0 is not implemented for the Tucker3 model")
        if sparse:
            raise NotImplementedError("sparse gradients are not implemented")
        if e_size != entity_slot_size:
            raise NotImplementedError("entity_embedding_size != entity_slot_size needs project_entity")
        if not (1 <= entity_slot_size <= MAX_SLOT and 1 <= r_size <= MAX_SLOT):
            raise NotImplementedError(f"Tucker3 slot / relation sizes outside 1..{MAX_SLOT}")
        self.train_data = train_data
        self.slot_size, self.relation_size = entity_slot_size, r_size
        # module construction order and initialisers = the reference's (model.py:389-430): same seed, same parameters
        self.entity_embedding = torch.nn.Embedding(train_data.entities_size, e_size, padding_idx=PAD)
        self.relation_embedding = torch.nn.Embedding(train_data.relations_size, r_size, padding_idx=PAD)
        layer = torch.nn.Linear(r_size, entity_slot_size ** 2, bias=False)
        torch.nn.init.xavier_normal_(layer.weight.data)
        self.relation_projection = torch.nn.Sequential(layer)
        self.project_entity, self.project_relation = False, True
        torch.nn.init.normal_(self.entity_embedding.weight.data, std=init_std)
        torch.nn.init.normal_(self.relation_embedding.weight.data, std=init_std)
        self.dropout, self.input_dropout = dropout, input_dropout
        self.relation_dropout = 0.0
        self.relation_input_dropout = input_dropout if relation_input_dropout is None else relation_input_dropout
        self.batch_norm, self.normalize, self.l2_reg = False, '', 0
        self._l2_reg_hook = None
        self.encode_in_torch = False
        self.dropout_seed, self.dropout_step = seed, 0
        self._engine = self._kernels = None

    # -- plumbing ----------------------------------------------------------------------------------------------
    @property
    def W(self):
        return self.relation_projection[0].weight.data

    def kernels(self) -> Tucker3Kernels:
        eng = self.engine()
        if self._kernels is None or self._kernels.engine is not eng:
            self._kernels = Tucker3Kernels(eng)
        return self._kernels

    def _rel_rows(self, rel, stream=H.STREAM_SP_REL, lookup=True):
        """masked rows of the relation table (relation_input_dropout), (b, r_e): what the projection is applied to"""
        return LookupBaseRelationEmbedder._encode(self, self.R, rel, stream, True, lookup)

    def encode_rel(self, rel, lookup=True):
        """(b, d^2) projected relation rows (model.py:482-490): gather + relation_input_dropout, then the Linear"""
        rows = self._rel_rows(rel, lookup=lookup)
        return ProjectRelFn.apply(rows.reshape(-1, self.relation_size), self.relation_projection[0].weight, self.kernels())

    def get_all_rel(self):
        """(|R| - min_relations_size, d^2) (model.py:512-517)"""
        rows = LookupBaseRelationEmbedder.get_all_rel(self)
        return ProjectRelFn.apply(rows.reshape(-1, self.relation_size), self.relation_projection[0].weight, self.kernels())

    # -- scores ------------------------------------------------------------------------------------------------
    def _prefix_score(self, batch: H.PrefixBatch, many=None):
        sp = batch.sp_subj is not None
        weight = self.relation_projection[0].weight
        with_graph = _wants_grad(self.entity_embedding.weight, self.relation_embedding.weight, weight, many)
        if with_graph and self.training:
            self.dropout_step += 1         # fresh masks per call, as each of the reference's encode calls draws them
        self._in_prefix_score = True
        try:
            if sp:
                ent, rel = self.encode_subj(batch.sp_subj), self._rel_rows(batch.sp_rel)
                cand = self.get_all_obj() if many is None else many
            else:
                cand = self.get_all_subj() if many is None else many
                rel, ent = self._rel_rows(batch.po_rel, H.STREAM_PO_REL), self.encode_obj(batch.po_obj)
        finally:
            self._in_prefix_score = False
        flat = lambda t: t.reshape(-1, t.shape[-1])      # noqa: E731
        if with_graph:
            return Tucker3PrefixScoreFn.apply(flat(ent), flat(rel), flat(cand), weight, self.kernels(), sp)
        with torch.no_grad():
            return Tucker3PrefixScoreFn.apply(flat(ent), flat(rel), flat(cand), weight, self.kernels(), sp)

    # -- training drivers ----------------------------------------------------------------------------------------------
    def train_step(self, loss="bce", lr=0.1, weight_decay=1e-10, eps=1e-8, label_smoothing=0.0, optimizer="adagrad", betas=(0.9, 0.999),
                   grad_clip=0.0):
        """The fused training driver: shares the module's parameters (updated in place).  optimizer / betas / grad_clip: as on
        FusedTrainStep."""
        return Tucker3TrainStep(self.E, self.R, self.W, loss=loss, lr=lr, weight_decay=weight_decay, eps=eps,
                                label_smoothing=label_smoothing, dropout=1.0 - (1.0 - self.input_dropout) * (1.0 - self.dropout),
                                relation_dropout=self.relation_input_dropout, seed=self.dropout_seed, engine=self.engine(),
                                optimizer=optimizer, betas=betas, grad_clip=grad_clip)

    def autograd_step(self, loss, label_smoothing):
        """the cached Tucker3TrainStep behind AddLossModule: shares the module's parameters; its optimizer is NOT used (the
        caller's torch optimizer steps the module parameters)"""
        st = getattr(self, "_ag_step", None)
        if st is None or st.loss != loss or st.label_smoothing != label_smoothing or st.E.data_ptr() != self.E.data_ptr() \
                or st.W.data_ptr() != self.W.data_ptr() or st.R.data_ptr() != self.R.data_ptr():
            st = self._ag_step = self.train_step(loss=loss, label_smoothing=label_smoothing)
        st.dropout = self.keep_prob_dropout(self.input_dropout, self.dropout)
        st.relation_dropout = self.keep_prob_dropout(self.relation_input_dropout, 0.0)
        # the gradient buffers of the last call went to autograd: fresh ones
        st.dE, st.dR, st.dW = torch.zeros_like(st.E), torch.zeros_like(st.R), torch.empty_like(st.W)
        st.steps = self.dropout_step
        self.dropout_step += 1
        return st

    def autograd_params_and_grads(self, st):
        return [self.entity_embedding.weight, self.relation_embedding.weight, self.relation_projection[0].weight], [st.dE, st.dR, st.dW]

    def optimizer_params_and_state(self, st):
        """For checkpoint.py, `st` = the driver train_step() returned: ([(parameter, the step's optimizer state tensors of it --
        (sum,) under Adagrad, (exp_avg, exp_avg_sq) under Adam --, True: the step moves it), ...] in self.parameters() order, the
        Adam device state word or None)."""
        found = {self.entity_embedding.weight: st.optimizer_state_of(st.E, st.sumE),
                 self.relation_embedding.weight: st.optimizer_state_of(st.R, st.sumR),
                 self.relation_projection[0].weight: st.optimizer_state_of(st.W, st.sumW)}
        return [(p, tuple(found[p]), True) for p in self.parameters()], st.adam_word()

    def loss_only(self, batch, kind, smoothing, all_outputs):
        """summed validation loss without gradients or dropout (AddLossModule under torch.no_grad(), trainer.py:363-369)"""
        step = self.dropout_step
        st = self.autograd_step(kind, smoothing)                            # (the cached step; no mask is drawn here)
        self.dropout_step = step
        return st.loss_only(batch, scores=all_outputs, normalizer=1.0)


class LookupTucker3RelationModel(RescalRelationScorer, ProjectedLookupRelationEmbedder):
    def __init__(self, **kwargs):
        kwargs.pop('project_relation', None)
        super().__init__(**kwargs, project_relation=True)


# registered like the reference's (model.py:1052-1066): getattr(Models, args["model"])
Models.LookupTucker3RelationModel = LookupTucker3RelationModel
