"""Host driver of the HIP hot path: torch tensors are containers (device memory + stream), all arithmetic
happens in libokge_hip.so through the C ABI of include/okge.h.

Reference call sites this module stands in for (paths relative to the reference checkout):
  AddLossModule.forward + backward    openkge/trainer.py:48-113, :217-234   -> HotPath.forward_backward
  *_prefix_score / _score             openkge/model.py:52-74, :198-229, :268-274 -> HotPath.score
  optimizer.step / zero_grad          utils/optim.py:139-160, trainer.py:229-244 -> HotPath.adagrad
  compute_metrics rank rule           openkge/dataset.py:423-446            -> HotPath.filtered_ranks
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field
from typing import Optional

import torch

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)

from . import _native as N


@dataclass
class DropoutSpec:
    """Dropout on gathered rows (model.py:461-462).  `keep` (uint8 [rows, d], device) overrides the
    counter-based Philox mask -- used to replay masks captured from the reference."""
    p: float = 0.0
    seed: int = 0
    stream: int = 0
    step: int = 0
    keep: Optional[torch.Tensor] = None
    step_dev: Optional[torch.Tensor] = None   # int32[1] on the device: the kernels read the step from it (graph replay)

    def fill(self, d: N.Dropout) -> N.Dropout:
        """every field of `d`, None included: a struct refilled in place keeps nothing of its last use"""
        d.p = float(self.p)
        d.seed = int(self.seed) & 0xFFFFFFFFFFFFFFFF
        d.stream = int(self.stream) & 0xFFFFFFFF
        d.step = int(self.step) & 0xFFFFFFFF
        d.keep = self.keep.data_ptr() if (self.keep is not None and self.p > 0) else None
        d.step_dev = self.step_dev.data_ptr() if self.step_dev is not None else None
        return d

    def c(self) -> N.Dropout:
        return self.fill(N.Dropout())


NO_DROP = DropoutSpec()

# slot sizes: the fused tile kernels (and everything built on them: the row-sparse step, the fused evaluation, top-k, the
# sharded phases) stop at TILE_MAX_SLOT; okge_score_prefixes, okge_train_forward_backward with dense gradients and
# okge_evaluate_batch go on to WIDE_MAX_SLOT on the wide path (csrc/okge_wide.hip)
TILE_MAX_SLOT, WIDE_MAX_SLOT = 512, 4096
ROWS_MAX_N = 1 << 20      # occurrence rows per tensor of the row calls (okge_adagrad_rows, okge_rows_to_dense, ...)

# OKGE_VALIDATE=1: check every id tensor against the table sizes before a call (one host sync per call).  The kernels
# trust their ids -- they live in device memory -- so a bad id is an out-of-bounds access; use this while integrating.
VALIDATE = os.environ.get("OKGE_VALIDATE") == "1"


def validate_ids(batch, n_ent, n_rel):
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return                                     # no host reads inside a graph capture
    def check(name, x, hi):
        if x is not None and x.numel():
            lo_, hi_ = int(x.min()), int(x.max())
            if lo_ < 0 or hi_ >= hi:
                raise N.OkgeError(f"{name}: ids span [{lo_}, {hi_}] but the table has {hi} rows")
    check("po_rel", batch.po_rel, n_rel)
    check("sp_rel", batch.sp_rel, n_rel)
    check("po_obj", batch.po_obj, n_ent)
    check("sp_subj", batch.sp_subj, n_ent)
    if batch.cand_table is None:
        check("cand_ids", batch.cand_ids, n_ent)
        if batch.cand_ids is None and (batch.cand_first < 0 or batch.cand_first + batch.n_cand > n_ent):
            raise N.OkgeError("candidate range outside the entity table")
    n_c = batch.n_candidates if batch.cand_table is None else batch.cand_table.shape[0]
    if batch.pos_row is not None and batch.pos_row.numel():
        live = batch.pos_row >= 0                  # (row -1, col INT32_MAX) pads a fixed-capacity list (GraphedTrainStep)
        check("pos_col", batch.pos_col[live], n_c)
        check("pos_row", batch.pos_row[live], batch.B)

# Philox stream ids: one per place the reference draws an independent Bernoulli mask
STREAMS = STREAM_CAND, STREAM_PO_ENT, STREAM_PO_REL, STREAM_SP_ENT, STREAM_SP_REL = 0, 1, 2, 3, 4


def dropout_specs(p_ent, p_rel, seed, step, step_dev=None):
    """the five masks of one step in stream order: the entity streams drop with p_ent, the relation streams with p_rel"""
    return tuple(DropoutSpec(p_rel if stream in (STREAM_PO_REL, STREAM_SP_REL) else p_ent, seed, stream, step, step_dev=step_dev)
                 for stream in STREAMS)


@dataclass
class PrefixBatch:
    """One batch in device memory: po rows (rel, obj) first, then sp rows (subj, rel); positives as
    (row, col) coordinates sorted by col (col = position in the candidate list)."""
    po_rel: Optional[torch.Tensor] = None   # int32 [n_po]
    po_obj: Optional[torch.Tensor] = None
    sp_subj: Optional[torch.Tensor] = None  # int32 [n_sp]
    sp_rel: Optional[torch.Tensor] = None
    pos_row: Optional[torch.Tensor] = None  # int32 [nnz]
    pos_col: Optional[torch.Tensor] = None
    cand_ids: Optional[torch.Tensor] = None  # int32 [N] or None for the range cand_first .. cand_first+N-1
    cand_first: int = 2
    n_cand: int = 0
    cand_table: Optional[torch.Tensor] = None  # scoring only: gather candidates from this (rows, d) table, not E
    cand_unique: bool = False               # cand_ids names every entity at most once (the collator's lists do)
    drop_po_ent: DropoutSpec = field(default_factory=DropoutSpec)
    drop_po_rel: DropoutSpec = field(default_factory=DropoutSpec)
    drop_sp_ent: DropoutSpec = field(default_factory=DropoutSpec)
    drop_sp_rel: DropoutSpec = field(default_factory=DropoutSpec)
    drop_cand: DropoutSpec = field(default_factory=DropoutSpec)

    def set_dropout(self, specs):
        """the five masks of one step, in the stream order dropout_specs(...) returns them"""
        self.drop_cand, self.drop_po_ent, self.drop_po_rel, self.drop_sp_ent, self.drop_sp_rel = specs
        return self

    @property
    def n_po(self):
        return 0 if self.po_rel is None else int(self.po_rel.numel())

    @property
    def n_sp(self):
        return 0 if self.sp_subj is None else int(self.sp_subj.numel())

    @property
    def B(self):
        return self.n_po + self.n_sp

    @property
    def nnz(self):
        return 0 if self.pos_row is None else int(self.pos_row.numel())

    @property
    def n_candidates(self):
        return int(self.n_cand if self.cand_ids is None else self.cand_ids.numel())


@dataclass
class Shard:
    """Rows [ent_lo, ent_hi) of the entity table live on this rank; cand_col0 = position of the first local
    candidate in the un-sharded candidate list (include/okge.h, okge_shard)."""
    ent_lo: int
    ent_hi: int
    cand_col0: int = 0

    def c(self) -> N.Shard:
        s = N.Shard()
        s.ent_lo, s.ent_hi, s.cand_col0 = int(self.ent_lo), int(self.ent_hi), int(self.cand_col0)
        return s


def _ptr(t):
    return None if t is None else t.data_ptr()


def n3_coef(l2_reg, dropout):
    """the factor of sum |x|^3 in the reference's hook: the rows are divided by `dropout` -- the probability, not the keep
    rate -- before the cube when it is > 0 (model.py:473-475)"""
    return float(l2_reg) / float(dropout) ** 3 if dropout > 0 else float(l2_reg)


def _i32(t, dev):
    if t is None:
        return None
    t = t.reshape(-1)
    if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
        t = t.to(device=dev, dtype=torch.int32).contiguous()
    return t


def occurrence_ids(dev, cand_ids, cand_first, n, po_obj, sp_subj, po_rel, sp_rel, out=None):
    """(ids_e, ids_r) int32 on the device: [candidate ids | po_obj | sp_subj] and [po_rel | sp_rel] -- the table row every
    occurrence row of okge_train_forward_backward(OKGE_TRAIN_ROW_GRADS) belongs to.  Index plumbing on the device, no host
    read; `out` = (ids_e, ids_r) buffers to fill in place (a captured graph refills them on replay)."""
    n_po = 0 if po_obj is None else int(po_obj.numel())
    n_sp = 0 if sp_subj is None else int(sp_subj.numel())
    if out is None:
        out = (torch.empty(n + n_po + n_sp, dtype=torch.int32, device=dev), torch.empty(n_po + n_sp, dtype=torch.int32, device=dev))
    ids_e, ids_r = out
    if cand_ids is None:
        torch.arange(cand_first, cand_first + n, dtype=torch.int32, device=dev, out=ids_e[:n])
    else:
        ids_e[:n].copy_(_i32(cand_ids, dev))
    if n_po:
        ids_e[n:n + n_po].copy_(_i32(po_obj, dev))
        ids_r[:n_po].copy_(_i32(po_rel, dev))
    if n_sp:
        ids_e[n + n_po:].copy_(_i32(sp_subj, dev))
        ids_r[n_po:].copy_(_i32(sp_rel, dev))
    return ids_e, ids_r


def _need_f32(dev, tensors, message, contiguous=True):
    for t in tensors:
        if t.dtype != torch.float32 or t.device != dev or (contiguous and not t.is_contiguous()):
            raise N.OkgeError(message)


def _need_i32(dev, tensors, message):
    for t in tensors:
        if t.dtype != torch.int32 or t.device != dev or not t.is_contiguous():
            raise N.OkgeError(message)


FREEZE_FLAGS = {None: 0, "entities": N.OKGE_TRAIN_FREEZE_ENTITIES, "relations": N.OKGE_TRAIN_FREEZE_RELATIONS}


def freeze_flag(freeze):
    """the OKGE_TRAIN_FREEZE_* bit of `freeze` (None, "entities" or "relations": the table that is not trained)"""
    try:
        return FREEZE_FLAGS[freeze]
    except (KeyError, TypeError):
        raise ValueError(f"freeze {freeze!r}: None, 'entities' or 'relations'") from None


def train_flags(grads_zero=False, loss_only=False, unique_candidates=False, distinct_prefix_rows=False, clear_grads=False,
                row_grads=False, freeze=None):
    """the OKGE_TRAIN_* word of okge_train_forward_backward / okge_n3_forward_backward / okge_train_tiles (include/okge.h);
    freeze: okge_train_forward_backward alone knows it"""
    return (0 if freeze is None else freeze_flag(freeze)) | (N.OKGE_TRAIN_GRADS_ZERO if grads_zero else 0) | (N.OKGE_TRAIN_LOSS_ONLY if loss_only else 0) | \
        (N.OKGE_TRAIN_UNIQUE_CANDIDATES if unique_candidates else 0) | (N.OKGE_TRAIN_DISTINCT_PREFIX_ROWS if distinct_prefix_rows else 0) | \
        (N.OKGE_TRAIN_CLEAR_GRADS if clear_grads else 0) | (N.OKGE_TRAIN_ROW_GRADS if row_grads else 0)


class PrefixCall:
    """The four argument structs of a prefix call (include/okge.h: okge_tables, okge_prefix_batch, okge_candidates,
    okge_positives) and the only Python code that knows their fields.  The step drivers keep one and refill it per call -- a
    0.14 ms step leaves the host ~100 us for everything, and building five dropout and four argument structs anew is a
    measurable part of that -- so every fill writes ALL the fields it owns, None and 0 included: nothing survives from the
    previous batch.  The fills read data_ptr(), shapes and numbers only (no engine, no GPU); the two launches take an engine.
    The tensors a fill was handed must live until the launch is issued."""

    def __init__(self):
        self.t, self.pb, self.c, self.pos = N.Tables(), N.PrefixBatch(), N.Candidates(), N.Positives()
        pb = self.pb
        self.drops = (self.c.drop, pb.drop_po_ent, pb.drop_po_rel, pb.drop_sp_ent, pb.drop_sp_rel)     # in STREAMS order
        self.n_po = self.n_sp = self.B = self.n = 0        # the shape fill_ids last wrote (B = n_po + n_sp rows, n candidates)

    def fill_tables(self, E, R, scorer, device):
        # (spelled out, not _need_f32: the step drivers pay for this fill on every step)
        if E.dtype != torch.float32 or R.dtype != torch.float32 or E.device != device or R.device != device \
                or not (E.is_contiguous() and R.is_contiguous()):
            raise N.OkgeError("embedding tables must be contiguous fp32 tensors on the engine's device")
        t = self.t
        t.E, t.R, t.n_ent, t.n_rel, t.d, t.scorer = E.data_ptr(), R.data_ptr(), E.shape[0], R.shape[0], E.shape[1], N.scorer_id(scorer)
        return t

    def fill_dropout(self, p_ent, p_rel, seed, step, step_dev=None):
        """the five Philox masks of one step (dropout_specs(...) in place)"""
        p_ent, p_rel, seed, step = float(p_ent), float(p_rel), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFF
        sd = None if step_dev is None else step_dev.data_ptr()
        for d, stream, p in zip(self.drops, STREAMS, (p_ent, p_ent, p_rel, p_ent, p_rel)):       # (cand, po_ent, po_rel, sp_ent, sp_rel)
            d.p, d.seed, d.stream, d.step, d.keep, d.step_dev = p, seed, stream, step, None, sd

    def fill_dropout_specs(self, specs):
        """five DropoutSpec objects in STREAMS order (they may carry replayed `keep` masks)"""
        for d, spec in zip(self.drops, specs):
            spec.fill(d)

    def fill_ids(self, po_rel, po_obj, sp_subj, sp_rel, cand_ids, cand_first, n_cand, pos_row=None, pos_col=None, cand_table=None):
        """the batch's ids: contiguous int32 tensors on the device or None; candidates are the list cand_ids or the range
        cand_first .. cand_first + n_cand - 1, gathered from cand_table (fp32 (rows, d)) instead of E when one is given"""
        pb, c, pos = self.pb, self.c, self.pos
        n_po = 0 if po_rel is None else po_rel.numel()
        n_sp = 0 if sp_subj is None else sp_subj.numel()
        pb.po_rel, pb.po_obj = (po_rel.data_ptr(), po_obj.data_ptr()) if n_po else (None, None)
        pb.sp_subj, pb.sp_rel = (sp_subj.data_ptr(), sp_rel.data_ptr()) if n_sp else (None, None)
        pb.n_po, pb.n_sp = n_po, n_sp
        n = int(n_cand) if cand_ids is None else cand_ids.numel()
        c.ids, c.first_id, c.n = (None if cand_ids is None else cand_ids.data_ptr()), int(cand_first), n
        c.table, c.table_rows = (None, 0) if cand_table is None else (cand_table.data_ptr(), cand_table.shape[0])
        nnz = 0 if pos_row is None else pos_row.numel()
        pos.row, pos.col, pos.nnz = (pos_row.data_ptr(), pos_col.data_ptr(), nnz) if nnz else (None, None, 0)
        self.n_po, self.n_sp, self.B, self.n = n_po, n_sp, n_po + n_sp, n

    def fill_batch(self, b: PrefixBatch, device):
        """ids and masks of a PrefixBatch of anything (host tensors, int64 ids, `keep` masks); -> the tensors the structs
        point into, to be held until the launch is issued"""
        keep = [_i32(x, device) for x in (b.po_rel, b.po_obj, b.sp_subj, b.sp_rel, b.cand_ids, b.pos_row, b.pos_col)]
        if b.cand_table is not None:
            _need_f32(device, (b.cand_table,), "candidate table must be a contiguous fp32 tensor on the engine's device")
        self.fill_ids(*keep[:5], b.cand_first, b.n_cand, keep[5], keep[6], b.cand_table)
        self.fill_dropout_specs((b.drop_cand, b.drop_po_ent, b.drop_po_rel, b.drop_sp_ent, b.drop_sp_rel))
        return keep

    def train(self, engine, loss, label_smoothing, normalizer, flags, loss_out, dE, dR, scores=None):
        """okge_train_forward_backward on the filled structs; normalizer None: B x N"""
        ws = engine.workspace(self.B, self.n, self.t.d, "train_rows" if flags & N.OKGE_TRAIN_ROW_GRADS else "train")
        if normalizer is None:
            normalizer = float(self.B) * float(self.n)
        N.check(engine.lib.okge_train_forward_backward(
            ctypes.byref(self.t), ctypes.byref(self.pb), ctypes.byref(self.c), ctypes.byref(self.pos), N.loss_id(loss),
            float(label_smoothing), float(normalizer), flags, loss_out.data_ptr(), _ptr(dE), _ptr(dR), _ptr(scores),
            0 if scores is None else scores.stride(0), ws.data_ptr(), engine._ws_bytes, engine._stream()), "okge_train_forward_backward")
        return loss_out

    def n3(self, engine, coef, cand_passes, normalizer, flags, reg_out, dE, dR):
        """okge_n3_forward_backward on the structs a train() call was just issued from (same rows, same masks)"""
        ws = engine.n3_workspace(self.B, self.n, min(self.t.d, WIDE_MAX_SLOT))
        if normalizer is None:
            normalizer = float(self.B) * float(self.n)
        N.check(engine.lib.okge_n3_forward_backward(
            ctypes.byref(self.t), ctypes.byref(self.pb), ctypes.byref(self.c), float(coef), int(cand_passes), float(normalizer),
            flags, reg_out.data_ptr(), _ptr(dE), _ptr(dR), ws.data_ptr(), engine._ws_bytes, engine._stream()), "okge_n3_forward_backward")
        return reg_out


class HotPath:
    """Owns the scratch workspace for one device and issues the C-ABI calls on torch's current stream."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise N.OkgeError("the open-KGE hot path runs on an MI355X (torch device 'cuda'); there is no CPU path")
        self.lib = N.lib()
        self._ws = None
        self._ws_bytes = 0
        # side scratch: buffers that outlive a call or run beside the one workspace (_side grows them)
        self._rows_ws = self._sb_ws = self._clip_ws = self._clip_multi_ws = self._ews = self._grad_rows = None

    # -- plumbing ------------------------------------------------------------------------------------
    def _stream(self):
        # the raw handle of torch's current stream on this device (torch.cuda.current_stream builds a Stream object:
        # ~5 us per call, and every library call asks)
        idx = self.device.index
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))

    def _grow(self, need):
        """the one workspace, reallocated only when a call needs more than it holds (the old block is dropped first)"""
        if need > self._ws_bytes:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws_bytes = need
        return self._ws

    def _side(self, name, need):
        """the side scratch buffer `name` with at least `need` bytes: grown, never shrunk"""
        buf = getattr(self, name)
        if buf is None or buf.numel() * buf.element_size() < need:
            buf = torch.empty(need, dtype=torch.uint8, device=self.device)
            setattr(self, name, buf)
        return buf

    def workspace(self, B, n_cand, d, kind="train"):
        """scratch for one call; kind 'score' (query block only) and 'lse' are much smaller than 'train'"""
        if kind == "score":
            need = int(self.lib.okge_score_workspace_bytes(B, d))
        elif kind == "lse":
            need = int(self.lib.okge_lse_workspace_bytes(B, n_cand, d))
        elif kind == "train_rows":
            need = int(self.lib.okge_train_row_grads_workspace_bytes(B, n_cand, d))
        else:
            need = int(self.lib.okge_train_workspace_bytes(B, n_cand, d))
        if need == 0:
            raise N.OkgeError(f"invalid problem size B={B} N={n_cand} d={d}")
        return self._grow(need)

    def _check(self, batch, E, R):
        if VALIDATE:
            validate_ids(batch, E.shape[0], R.shape[0])

    def _tables(self, E, R, scorer):
        return PrefixCall().fill_tables(E, R, scorer, self.device)

    def _filled(self, b: PrefixBatch):
        """-> (a fresh PrefixCall holding the batch, the int32 tensors it points into)"""
        call = PrefixCall()
        return call, call.fill_batch(b, self.device)

    def _batch(self, b: PrefixBatch):
        call, keep = self._filled(b)
        return call.pb, call.c, keep

    def _positives(self, b: PrefixBatch):
        call, keep = self._filled(b)
        return call.pos, keep

    # -- entry points -------------------------------------------------------------------------------
    def score(self, E, R, scorer, batch: PrefixBatch, out=None):
        """(B, N) scores of every prefix against every candidate (eval / *_prefix_score)."""
        self._check(batch, E, R)
        pb, c, keep = self._batch(batch)
        t = self._tables(E, R, scorer)
        B, n = batch.B, c.n
        ws = self.workspace(B, n, t.d, "score")
        if out is None:
            ld = (n + 3) // 4 * 4
            out = torch.empty((B, ld), dtype=torch.float32, device=self.device)[:, :n]
        N.check(self.lib.okge_score_prefixes(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), out.data_ptr(),
                                             out.stride(0), ws.data_ptr(), self._ws_bytes, self._stream()),
                "okge_score_prefixes")
        del keep
        return out

    def forward_backward(self, E, R, scorer, batch: PrefixBatch, dE, dR, loss="bce", label_smoothing=0.0,
                         normalizer=None, loss_out=None, scores=None, grads_zero=False, loss_only=False,
                         distinct_prefix_rows=False, clear_grads=False, row_grads=False, freeze=None):
        """Fused forward + loss + backward; accumulates into dE / dR (clear_grads: into whatever-they-held buffers that the
        call itself clears, okge.h OKGE_TRAIN_CLEAR_GRADS); returns the summed loss as a device double[1] tensor (no host sync).
        row_grads: dE (N + B, d) / dR (B, d) are occurrence-row buffers, every row stored once (okge.h OKGE_TRAIN_ROW_GRADS).
        freeze ("entities" / "relations", okge.h OKGE_TRAIN_FREEZE_*): that table is not trained, its buffer may be None and is
        not touched; with "entities" the candidate-gradient product is not computed."""
        self._check(batch, E, R)
        call, keep = self._filled(batch)
        d = call.fill_tables(E, R, scorer, self.device).d
        B, n = call.B, call.n
        if row_grads:
            if loss_only or dE is None or dR is None or tuple(dE.shape) != (n + B, d) or tuple(dR.shape) != (B, d) \
                    or not dE.is_contiguous() or not dR.is_contiguous():
                raise N.OkgeError(f"row_grads: dE must be a contiguous ({n + B}, {d}) and dR a ({B}, {d}) fp32 buffer")
        if loss_out is None:
            loss_out = torch.empty(1, dtype=torch.float64, device=self.device)
        flags = train_flags(grads_zero=grads_zero, loss_only=loss_only, unique_candidates=batch.cand_unique,
                            distinct_prefix_rows=distinct_prefix_rows, clear_grads=clear_grads, row_grads=row_grads, freeze=freeze)
        call.train(self, loss, label_smoothing, normalizer, flags, loss_out, dE, dR, scores)
        del keep
        return loss_out

    def n3_workspace(self, B, n_cand, d):
        """scratch of okge_n3_forward_backward: it runs after the step on the same stream, so it shares the step's workspace"""
        need = int(self.lib.okge_n3_workspace_bytes(B, n_cand, d))
        if need == 0:
            raise N.OkgeError(f"invalid problem size B={B} N={n_cand} d={d}")
        return self._grow(need)

    def n3_forward_backward(self, E, R, scorer, batch: PrefixBatch, dE, dR, coef, cand_passes=1, normalizer=None, reg_out=None,
                            loss_only=False, distinct_prefix_rows=False, row_grads=False):
        """The N3 regulariser (`l2_reg`, model.py:471-479) of the batch's rows under the batch's dropout masks:
        reg_out (device double[1]) = coef * (cand_passes * sum over the candidate rows + sum over the prefix rows) of |x|^3, and
        its gradient / normalizer ADDED to dE / dR -- issue it after forward_backward with the same batch and buffers
        (okge.h, okge_n3_forward_backward).  coef = n3_coef(l2_reg, dropout)."""
        self._check(batch, E, R)
        call, keep = self._filled(batch)
        call.fill_tables(E, R, scorer, self.device)
        if reg_out is None:
            reg_out = torch.empty(1, dtype=torch.float64, device=self.device)
        flags = train_flags(loss_only=loss_only, unique_candidates=batch.cand_unique, distinct_prefix_rows=distinct_prefix_rows,
                            row_grads=row_grads)
        call.n3(self, coef, cand_passes, normalizer, flags, reg_out, dE, dR)
        del keep
        return reg_out

    # -- entity-sharded phases (include/okge.h: okge_encode_queries / okge_train_tiles / okge_prefix_backward) ----
    def query_shape(self, B, d):
        return int(self.lib.okge_query_rows(B)), int(self.lib.okge_query_ld(d))

    def encode_queries(self, E_local, R, scorer, batch: PrefixBatch, shard: Shard, out=None):
        """-> buffer [2][rows][ld]: out[0] = folded queries, out[1] = masked prefix entity rows; rows of prefixes
        whose entity another rank owns are zero (the caller all-reduces the buffer)."""
        pb, c, keep = self._batch(batch)
        t = self._tables(E_local, R, scorer)
        rows, ld = self.query_shape(batch.B, t.d)
        if out is None:
            out = torch.empty((2, rows, ld), dtype=torch.float32, device=self.device)
        sh = shard.c()
        N.check(self.lib.okge_encode_queries(ctypes.byref(t), ctypes.byref(sh), ctypes.byref(pb), out[0].data_ptr(), ld,
                                             out[1].data_ptr(), self._stream()), "okge_encode_queries")
        del keep
        return out

    def encode_entity_rows(self, E_local, R, scorer, batch: PrefixBatch, shard: Shard, out=None):
        """-> [rows][ld] masked prefix entity rows of the prefixes whose entity lives here, zeros elsewhere (the
        caller all-reduces the buffer, then every rank calls fold_queries)."""
        pb, c, keep = self._batch(batch)
        t = self._tables(E_local, R, scorer)
        rows, ld = self.query_shape(batch.B, t.d)
        if out is None:
            out = torch.empty((rows, ld), dtype=torch.float32, device=self.device)
        sh = shard.c()
        N.check(self.lib.okge_encode_queries(ctypes.byref(t), ctypes.byref(sh), ctypes.byref(pb), None, ld,
                                             out.data_ptr(), self._stream()), "okge_encode_queries")
        del keep
        return out

    def fold_queries(self, E_local, R, scorer, batch: PrefixBatch, ent_rows, out=None):
        """query block from exchanged masked entity rows and the replicated relation table"""
        pb, c, keep = self._batch(batch)
        t = self._tables(E_local, R, scorer)
        if out is None:
            out = torch.empty_like(ent_rows)
        N.check(self.lib.okge_fold_queries(ctypes.byref(t), ctypes.byref(pb), ent_rows.data_ptr(), ent_rows.stride(0),
                                           out.data_ptr(), self._stream()), "okge_fold_queries")
        del keep
        return out

    def train_tiles(self, E_local, R, scorer, Q, batch: PrefixBatch, shard: Shard, dE, dQ, n_cand_global, loss="bce",
                    label_smoothing=0.0, normalizer=None, loss_out=None, grads_zero=False, row_lse=None, *, loss_only=False,
                    B=None):
        """Local candidates only: batch.cand_first / n_cand are LOCAL row indices, batch.pos_col GLOBAL columns.
        KL loss: `row_lse` = log-sum-exp of every row's scores over ALL shards' candidates.  loss_only: no gradients.
        B: query rows in Q, for a batch that names candidates and positives only (default: the batch's rows)."""
        call, keep = self._filled(batch)
        t, c, pos = call.fill_tables(E_local, R, scorer, self.device), call.c, call.pos
        B, n = batch.B if B is None else int(B), c.n
        ws = self.workspace(B, n, t.d)
        if normalizer is None:
            normalizer = float(B) * float(n_cand_global)
        if loss_out is None:
            loss_out = torch.empty(1, dtype=torch.float64, device=self.device)
        sh = shard.c()
        N.check(self.lib.okge_train_tiles(
            ctypes.byref(t), ctypes.byref(sh), Q.data_ptr(), Q.stride(0), B, ctypes.byref(c), ctypes.byref(pos),
            N.loss_id(loss), float(label_smoothing), float(normalizer), int(n_cand_global),
            train_flags(grads_zero=grads_zero, loss_only=loss_only, unique_candidates=batch.cand_unique), _ptr(row_lse),
            loss_out.data_ptr(), dE.data_ptr(), dQ.data_ptr(), ws.data_ptr(), self._ws_bytes, self._stream()), "okge_train_tiles")
        del keep
        return loss_out

    def score_queries(self, E_local, R, scorer, Q, B, batch: PrefixBatch, shard: Shard, out=None):
        """(B, n_local) scores of precomputed query rows against the local candidates."""
        pb, c, keep = self._batch(batch)
        t = self._tables(E_local, R, scorer)
        if out is None:
            out = torch.empty((B, (c.n + 3) // 4 * 4), dtype=torch.float32, device=self.device)[:, :c.n]
        sh = shard.c()
        N.check(self.lib.okge_score_queries(ctypes.byref(t), ctypes.byref(sh), Q.data_ptr(), Q.stride(0), B,
                                            ctypes.byref(c), out.data_ptr(), out.stride(0), self._stream()),
                "okge_score_queries")
        del keep
        return out

    def row_logsumexp(self, E_local, R, scorer, Q, B, batch: PrefixBatch, shard: Shard):
        """(B,) log-sum-exp of each query row's scores over the local candidates (scores are not materialised)."""
        pb, c, keep = self._batch(batch)
        t = self._tables(E_local, R, scorer)
        ws = self.workspace(B, c.n, t.d, "lse")
        out = torch.empty(B, dtype=torch.float32, device=self.device)
        sh = shard.c()
        N.check(self.lib.okge_row_logsumexp(ctypes.byref(t), ctypes.byref(sh), Q.data_ptr(), Q.stride(0), B,
                                            ctypes.byref(c), out.data_ptr(), ws.data_ptr(), self._ws_bytes,
                                            self._stream()), "okge_row_logsumexp")
        del keep
        return out

    # -- top-k link prediction (include/okge.h: okge_topk_prefixes / okge_topk_queries / okge_topk_merge) ----------------
    def _topk_workspace(self, B, n, d, k, range_n):
        need = int(self.lib.okge_topk_workspace_bytes(B, n, d, int(k), int(range_n)))
        if need == 0:
            raise N.OkgeError(f"invalid top-k problem B={B} N={n} d={d} k={k} range_n={range_n} (1 <= k <= 64, d <= 512)")
        return self._grow(need)

    def _filter(self, filt_ptr, filt_col):
        """-> (filt_ptr int64, filt_col int32, n_filter) on the device, or (None, None, 0)"""
        if filt_ptr is None or filt_col is None or int(filt_col.numel()) == 0:
            return None, None, 0
        fp = filt_ptr.reshape(-1)
        if fp.dtype != torch.int64 or fp.device != self.device or not fp.is_contiguous():
            fp = fp.to(device=self.device, dtype=torch.int64).contiguous()
        fc = _i32(filt_col, self.device)
        return fp, fc, int(fc.numel())

    def topk_prefixes(self, E, R, scorer, batch: PrefixBatch, k, filt_ptr=None, filt_col=None, range_n=0):
        """-> (scores (B, k) fp32, cols (B, k) int32, ids (B, k) int32): every row's k best unfiltered candidates in the total
        order of include/okge.h, without the (B, N) score block.  filt_ptr / filt_col: CSR of each row's excluded columns."""
        self._check(batch, E, R)
        pb, c, keep = self._batch(batch)
        t = self._tables(E, R, scorer)
        B, k = batch.B, int(k)
        ws = self._topk_workspace(B, c.n, t.d, k, range_n) if 1 <= k <= 64 and t.d <= 512 else self.workspace(B, c.n, min(t.d, 512), "score")
        fp, fc, nf = self._filter(filt_ptr, filt_col)
        shape = (B, max(k, 1))
        scores = torch.empty(shape, dtype=torch.float32, device=self.device)
        cols = torch.empty(shape, dtype=torch.int32, device=self.device)
        ids = torch.empty(shape, dtype=torch.int32, device=self.device)
        N.check(self.lib.okge_topk_prefixes(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), k, _ptr(fp), _ptr(fc), nf,
                                            int(range_n), scores.data_ptr(), cols.data_ptr(), ids.data_ptr(), ws.data_ptr(),
                                            self._ws_bytes, self._stream()), "okge_topk_prefixes")
        del keep
        return scores, cols, ids

    def topk_queries(self, E_local, R, scorer, Q, B, batch: PrefixBatch, shard: Shard, k, filt_ptr=None, filt_col=None, range_n=0):
        """-> (scores (B, k), cols (B, k)) of precomputed query rows against the LOCAL candidates; columns and filter columns
        are global (shard.cand_col0 + local position)."""
        pb, c, keep = self._batch(batch)
        t = self._tables(E_local, R, scorer)
        k = int(k)
        ws = self._topk_workspace(B, c.n, t.d, k, range_n)
        fp, fc, nf = self._filter(filt_ptr, filt_col)
        scores = torch.empty((B, k), dtype=torch.float32, device=self.device)
        cols = torch.empty((B, k), dtype=torch.int32, device=self.device)
        sh = shard.c()
        N.check(self.lib.okge_topk_queries(ctypes.byref(t), ctypes.byref(sh), Q.data_ptr(), Q.stride(0), B, ctypes.byref(c), k,
                                           _ptr(fp), _ptr(fc), nf, int(range_n), scores.data_ptr(), cols.data_ptr(),
                                           ws.data_ptr(), self._ws_bytes, self._stream()), "okge_topk_queries")
        del keep
        return scores, cols

    def topk_merge(self, scores, cols):
        """(n_lists, B, k) lists -> the (B, k) list of their union in the same order"""
        n_lists, B, k = scores.shape
        scores, cols = scores.contiguous(), cols.contiguous()
        out_s = torch.empty((B, k), dtype=torch.float32, device=self.device)
        out_c = torch.empty((B, k), dtype=torch.int32, device=self.device)
        N.check(self.lib.okge_topk_merge(scores.data_ptr(), cols.data_ptr(), n_lists, B, k, out_s.data_ptr(), out_c.data_ptr(),
                                         self._stream()), "okge_topk_merge")
        return out_s, out_c

    def prefix_backward(self, E_local, R, scorer, batch: PrefixBatch, shard: Shard, dQ, ent_rows, dE, dR, rel_segments=None):
        """rel_segments: sharded.RowSegments (make_row_segments) -- relation and / or entity gradients by sorted segments
        instead of float atomics"""
        pb, c, keep = self._batch(batch)
        t = self._tables(E_local, R, scorer)
        sh = shard.c()
        if rel_segments is not None:
            sg = rel_segments
            grad_rows = self._side("_grad_rows", 2 * dQ.shape[0] * dQ.stride(0) * dQ.element_size())     # [2][rows][ld] as dQ
            r_o, r_p = sg.rel if sg.rel is not None else (None, None)
            e_o, e_p = sg.ent if sg.ent is not None else (None, None)
            N.check(self.lib.okge_prefix_backward_segmented(ctypes.byref(t), ctypes.byref(sh), ctypes.byref(pb), dQ.data_ptr(),
                                                            dQ.stride(0), _ptr(ent_rows), _ptr(r_o), _ptr(r_p),
                                                            0 if r_p is None else int(r_p.numel()) - 1, _ptr(e_o), _ptr(e_p),
                                                            0 if e_p is None else int(e_p.numel()) - 1, grad_rows.data_ptr(),
                                                            dE.data_ptr(), dR.data_ptr(), self._stream()),
                    "okge_prefix_backward_segmented")
            del keep
            return
        N.check(self.lib.okge_prefix_backward(ctypes.byref(t), ctypes.byref(sh), ctypes.byref(pb), dQ.data_ptr(),
                                              dQ.stride(0), _ptr(ent_rows), dE.data_ptr(), dR.data_ptr(),
                                              self._stream()), "okge_prefix_backward")
        del keep

    def score_triples(self, scorer, subj, rel, obj):
        """(b, 1) scores of b encoded triples (rows (b, d), last dim contiguous): triple_score (model.py:178-179)."""
        rows = [x.reshape(-1, x.shape[-1]) for x in (subj, rel, obj)]
        b, d = rows[0].shape
        message = "triple rows must be fp32 (b, d) on the engine's device with a contiguous last dim"
        _need_f32(self.device, rows, message, contiguous=False)
        if any(x.stride(1) != 1 or x.shape != (b, d) for x in rows):
            raise N.OkgeError(message)
        out = torch.empty((b, 1), dtype=torch.float32, device=self.device)
        N.check(self.lib.okge_score_triples(N.scorer_id(scorer), rows[0].data_ptr(), rows[0].stride(0), rows[1].data_ptr(), rows[1].stride(0),
                                            rows[2].data_ptr(), rows[2].stride(0), b, d, out.data_ptr(), self._stream()),
                "okge_score_triples")
        return out

    def encode_rows(self, table, ids=None, first_id=0, n=None, drop: DropoutSpec = NO_DROP, out=None):
        """dropout(table[ids]) -> (n, d): LookupBaseRelationEmbedder._encode (model.py:455-480)."""
        ids = _i32(ids, self.device)
        n = int(ids.numel()) if ids is not None else int(n)
        d = table.shape[1]
        if out is None:
            out = torch.empty((n, d), dtype=torch.float32, device=self.device)
        dc = drop.c()
        N.check(self.lib.okge_encode_rows(table.data_ptr(), table.shape[0], d, _ptr(ids), int(first_id), n,
                                          ctypes.byref(dc), out.data_ptr(), out.stride(0), self._stream()),
                "okge_encode_rows")
        return out

    def prefix_score_backward(self, scorer, sp, g, ent, rel, cand, need_ent=True, need_rel=True, need_cand=True):
        """(d_ent, d_rel, d_cand) of scores = fold(ent, rel) . cand^T from the dense (b, n) gradient g (okge_prefix_score_backward)"""
        b, n = g.shape
        d = cand.shape[1]
        ws = self._side("_sb_ws", int(self.lib.okge_prefix_score_backward_workspace_bytes(b, n, d)))
        out = [torch.empty((b, d), dtype=torch.float32, device=self.device) if need_ent else None,
               torch.empty((b, d), dtype=torch.float32, device=self.device) if need_rel else None,
               torch.empty((n, d), dtype=torch.float32, device=self.device) if need_cand else None]
        N.check(self.lib.okge_prefix_score_backward(N.scorer_id(scorer), 1 if sp else 0, g.data_ptr(), g.stride(0), b, n, ent.data_ptr(),
                                                    ent.stride(0), rel.data_ptr(), rel.stride(0), cand.data_ptr(), cand.stride(0), d,
                                                    _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), ws.data_ptr(), ws.numel(), self._stream()),
                "okge_prefix_score_backward")
        return out

    def scatter_rows(self, rows, ids, first_id, table_grad, drop: DropoutSpec = NO_DROP):
        """table_grad[id] += masked rows of the positions naming id, summed in sorted-position order (okge_scatter_rows)"""
        n, d = rows.shape
        order = None
        if ids is not None:
            ids = _i32(ids, self.device)
            order = torch.argsort(ids, stable=True).to(torch.int32)          # (index plumbing; the sums are the kernel's)
        dc = drop.c()
        N.check(self.lib.okge_scatter_rows(rows.data_ptr(), rows.stride(0), _ptr(ids), _ptr(order), int(first_id), n, d, ctypes.byref(dc),
                                           table_grad.data_ptr(), table_grad.shape[0], self._stream()), "okge_scatter_rows")
        return table_grad

    def scale_(self, x, alpha_dev):
        """x *= alpha (device fp32 scalar) in place."""
        N.check(self.lib.okge_scale_inplace(x.data_ptr(), x.numel(), alpha_dev.data_ptr(), self._stream()),
                "okge_scale_inplace")
        return x

    def rescale_gradients_(self, g0, g1, alpha_dev, applied):
        """g0, g1 *= alpha / applied (alpha: device fp32 scalar) in ONE launch; free when the two are the same number.
        g1 None: g0 alone"""
        N.check(self.lib.okge_rescale_gradients(g0.data_ptr(), g0.numel(), _ptr(g1), 0 if g1 is None else g1.numel(), alpha_dev.data_ptr(),
                                                float(applied), self._stream()), "okge_rescale_gradients")

    def adagrad(self, p, g, state_sum, lr, weight_decay=1e-10, eps=1e-8, zero_grad=True):
        N.check(self.lib.okge_adagrad_step(p.data_ptr(), g.data_ptr(), state_sum.data_ptr(), p.numel(), float(lr),
                                           float(weight_decay), float(eps), 1 if zero_grad else 0, self._stream()),
                "okge_adagrad_step")

    def adagrad2(self, p0, g0, s0, p1, g1, s1, lr, weight_decay=1e-10, eps=1e-8, zero_grad=True):
        """Both tables in one launch.  zero_grad: False/0 none, True/1 both, 2 only g1 (see include/okge.h)."""
        N.check(self.lib.okge_adagrad_step2(p0.data_ptr(), g0.data_ptr(), s0.data_ptr(), p0.numel(), p1.data_ptr(),
                                            g1.data_ptr(), s1.data_ptr(), p1.numel(), float(lr), float(weight_decay),
                                            float(eps), int(zero_grad), self._stream()), "okge_adagrad_step2")

    def adagrad_multi(self, tensors, lr, weight_decay=1e-10, eps=1e-8):
        """One launch over up to four (p, g, state_sum[, touched_map, stamp]) tuples, gradients cleared in the sweep
        (okge_adagrad_multi): a tensor with a touched-row byte map skips the gradient rows the map does not stamp."""
        arr = (N.AdagradTensor * len(tensors))()
        for a, t in zip(arr, tensors):
            p, g, s = t[:3]
            a.p, a.g, a.state_sum, a.n, a.zero_grad = p.data_ptr(), g.data_ptr(), s.data_ptr(), p.numel(), 1
            if len(t) > 3 and t[3] is not None:
                a.row_touched, a.row_len, a.touched_stamp = t[3].data_ptr(), p.shape[1], int(t[4])
        N.check(self.lib.okge_adagrad_multi(arr, len(tensors), float(lr), float(weight_decay), float(eps), self._stream()),
                "okge_adagrad_multi")

    def adagrad_rows(self, p, state_sum, ids, g, lr, eps=1e-8, second=None):
        """okge_adagrad_rows: the occurrence rows g (n, row_len) of the int32 device ids are coalesced per id in ascending
        position and the named rows of p / state_sum take one Adagrad step (weight_decay = 0); every other row is left alone.
        second: another (p, state_sum, ids, g) for the same launches."""
        tensors = [(p, state_sum, ids, g)] + ([tuple(second)] if second is not None else [])
        arr = (N.RowsTensor * len(tensors))()
        for a, (p_, s_, i_, g_) in zip(arr, tensors):
            _need_i32(self.device, (i_,), "adagrad_rows: ids must be a contiguous int32 tensor on the engine's device")
            _need_f32(self.device, (p_, s_, g_), "adagrad_rows: fp32 tensors on the engine's device", contiguous=False)
            if p_.dim() != 2 or not p_.is_contiguous() or not s_.is_contiguous() or s_.shape != p_.shape:
                raise N.OkgeError("adagrad_rows: p and state_sum must be contiguous (rows, row_len) tensors of one shape")
            a.p, a.state_sum = p_.data_ptr(), s_.data_ptr()
            self._fill_rows(a, "adagrad_rows", p_, i_, g_)
        ws = self._rows_scratch(arr, self.lib.okge_adagrad_rows_workspace_bytes)
        N.check(self.lib.okge_adagrad_rows(arr, len(tensors), float(lr), float(eps), ws.data_ptr(), ws.numel(), self._stream()),
                "okge_adagrad_rows")

    def rows_to_dense(self, tensors, accumulate=False):
        """okge_rows_to_dense: one or two (dense, ids, g) -- the occurrence rows g (n, row_len) of the int32 device ids are added
        per id in ascending position, sequentially in fp32, and written to the named rows of the dense gradient table `dense`
        (rows, row_len).  accumulate=False: those rows are overwritten (every other row must already be zero); True: each named
        row continues the chain from what it holds.  Rows no id names are not written; no float atomics."""
        arr = (N.RowsTensor * len(tensors))()
        for a, (p_, i_, g_) in zip(arr, tensors):
            _need_i32(self.device, (i_,), "rows_to_dense: ids must be a contiguous int32 tensor on the engine's device")
            _need_f32(self.device, (p_, g_), "rows_to_dense: fp32 tensors on the engine's device", contiguous=False)
            if p_.dim() != 2 or not p_.is_contiguous():
                raise N.OkgeError("rows_to_dense: the dense gradient must be a contiguous (rows, row_len) tensor")
            a.p = p_.data_ptr()
            self._fill_rows(a, "rows_to_dense", p_, i_, g_)
        ws = self._rows_scratch(arr, self.lib.okge_rows_to_dense_workspace_bytes)
        N.check(self.lib.okge_rows_to_dense(arr, len(tensors), N.OKGE_ROWS_ACCUMULATE if accumulate else N.OKGE_ROWS_STORE,
                                            ws.data_ptr(), ws.numel(), self._stream()), "okge_rows_to_dense")

    def _fill_rows(self, a, who, p, ids, g):
        """the (ids, g, ld_g, n, table_rows, row_len) block the three row-tensor structs share; g None: no gradient rows"""
        n, row_len = int(ids.numel()), int(p.shape[1])
        a.ids, a.n, a.table_rows, a.row_len, a.ld_g = ids.data_ptr(), n, int(p.shape[0]), row_len, row_len
        if g is not None:
            if n and (g.dim() != 2 or g.shape[0] != n or g.shape[1] != row_len or g.stride(1) != 1):
                raise N.OkgeError(f"{who}: g must hold one row of row_len floats per id, last dim contiguous")
            a.g = g.data_ptr()
            if n > 1:
                a.ld_g = int(g.stride(0))

    def _rows_scratch(self, arr, size):
        """the sort-key scratch of a row-tensor array of one or two tensors (size: the entry point's *_workspace_bytes)"""
        ns = [int(a.n) for a in arr] + [0]
        return self._side("_rows_ws", max(int(size(ns[0], ns[1])), 256))

    @staticmethod
    def adam_state(device, step=0):
        """the device state of one Adam tensor (okge_adam_tensor.state): int32[4] = [steps taken, scratch x 3]"""
        st = torch.zeros(4, dtype=torch.int32, device=device)
        if step:
            st[0] = int(step)
        return st

    def _adam_tensors(self, struct, tensors, who):
        """(p, g, exp_avg, exp_avg_sq, state, ...) tuples -> an array of `struct` with the fields okge_adam_tensor and
        okge_adam_multi_tensor share"""
        arr = (struct * len(tensors))()
        state_message = f"{who}: the state is a contiguous int32[4] tensor on the engine's device (HotPath.adam_state)"
        for a, (p, g, m, v, st) in zip(arr, (t[:5] for t in tensors)):
            _need_f32(self.device, (p, g, m, v), f"{who}: contiguous fp32 tensors on the engine's device")
            if g.numel() != p.numel() or m.numel() != p.numel() or v.numel() != p.numel():
                raise N.OkgeError(f"{who}: p, g, exp_avg and exp_avg_sq must have one size")
            _need_i32(self.device, (st,), state_message)
            if st.numel() != 4:
                raise N.OkgeError(state_message)
            a.p, a.g, a.exp_avg, a.exp_avg_sq, a.state, a.n = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), p.numel()
        return arr

    def adam(self, tensors, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, zero_grad=True):
        """okge_adam_step: torch.optim.Adam's update (no amsgrad, coupled weight decay) on one or two (p, g, exp_avg, exp_avg_sq,
        state) tuples in one sweep; each state (adam_state) advances by one step on the device.  zero_grad as adagrad2."""
        arr = self._adam_tensors(N.AdamTensor, tensors, "adam")
        N.check(self.lib.okge_adam_step(arr, len(tensors), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                        int(zero_grad), self._stream()), "okge_adam_step")

    def adam_multi(self, tensors, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """okge_adam_multi: okge_adam_step's update on up to four (p, g, exp_avg, exp_avg_sq, state[, touched_map, stamp]) tuples in
        one sweep, gradients cleared; a tensor with a touched-row byte map takes g = 0 on the rows the map does not stamp, whose
        gradient rows are neither read nor cleared.  Every distinct state advances by one step on the device."""
        arr = self._adam_tensors(N.AdamMultiTensor, tensors, "adam_multi")
        for a, t in zip(arr, tensors):
            if len(t) > 5 and t[5] is not None:
                a.row_touched, a.row_len, a.touched_stamp = t[5].data_ptr(), t[0].shape[1], int(t[6])
        N.check(self.lib.okge_adam_multi(arr, len(tensors), float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                         self._stream()), "okge_adam_multi")

    def clip_grad_norm_multi_(self, tensors, max_norm, norm_out=None):
        """okge_clip_grad_norm_multi: torch.nn.utils.clip_grad_norm_ over up to eight gradient tensors, in place; tensors: g or
        (g, touched_map, stamp) -- gradient rows a map does not stamp are neither read nor written.  norm_out: device double[1]."""
        arr = (N.GradTensor * len(tensors))()
        for a, t in zip(arr, tensors):
            g, touched, stamp = t if isinstance(t, (tuple, list)) else (t, None, 0)
            _need_f32(self.device, (g,), "clip_grad_norm_multi: contiguous fp32 tensors on the engine's device")
            a.g, a.n = g.data_ptr(), g.numel()
            if touched is not None:
                a.row_touched, a.row_len, a.touched_stamp = touched.data_ptr(), g.shape[1], int(stamp)
        ws = self._side("_clip_multi_ws", int(self.lib.okge_clip_grad_norm_multi_workspace_bytes()))
        N.check(self.lib.okge_clip_grad_norm_multi(arr, len(tensors), float(max_norm), _ptr(norm_out), ws.data_ptr(), ws.numel(),
                                                   self._stream()), "okge_clip_grad_norm_multi")

    def adam_rows(self, tensors, lr, betas=(0.9, 0.999), eps=1e-8):
        """okge_adam_rows: torch.optim.SparseAdam's update on one or two (p, exp_avg, exp_avg_sq, state, ids, g) tuples -- the
        occurrence rows g (n, row_len) of the int32 device ids are coalesced per id in ascending position and only the named rows
        of p and the two moments move; every state advances by one step, also where n = 0."""
        arr = (N.AdamRowsTensor * len(tensors))()
        for a, (p_, m_, v_, st_, i_, g_) in zip(arr, tensors):
            _need_i32(self.device, (i_, st_), "adam_rows: ids and state must be contiguous int32 tensors on the engine's device")
            _need_f32(self.device, (p_, m_, v_, g_), "adam_rows: fp32 tensors on the engine's device", contiguous=False)
            if p_.dim() != 2 or not (p_.is_contiguous() and m_.is_contiguous() and v_.is_contiguous()) or m_.shape != p_.shape or \
                    v_.shape != p_.shape or st_.numel() != 4:
                raise N.OkgeError("adam_rows: p, exp_avg and exp_avg_sq must be contiguous (rows, row_len) tensors of one shape, state int32[4]")
            a.p, a.exp_avg, a.exp_avg_sq, a.state = p_.data_ptr(), m_.data_ptr(), v_.data_ptr(), st_.data_ptr()
            self._fill_rows(a, "adam_rows", p_, i_, g_)
        ws = self._rows_scratch(arr, self.lib.okge_adam_rows_workspace_bytes)
        N.check(self.lib.okge_adam_rows(arr, len(tensors), float(lr), float(betas[0]), float(betas[1]), float(eps), ws.data_ptr(),
                                        ws.numel(), self._stream()), "okge_adam_rows")

    def _rows_decay_tensors(self, tensors, who):
        """(p, state_sum, ids, g or None, row_steps) tuples -> the okge_rows_decay_tensor array"""
        arr = (N.RowsDecayTensor * len(tensors))()
        for a, (p_, s_, i_, g_, st_) in zip(arr, tensors):
            _need_i32(self.device, (i_, st_), f"{who}: ids and row_steps must be contiguous int32 tensors on the engine's device")
            _need_f32(self.device, (p_, s_) + (() if g_ is None else (g_,)), f"{who}: fp32 tensors on the engine's device", contiguous=False)
            if p_.dim() != 2 or not p_.is_contiguous() or not s_.is_contiguous() or s_.shape != p_.shape or st_.numel() != p_.shape[0]:
                raise N.OkgeError(f"{who}: p and state_sum must be contiguous (rows, row_len) tensors of one shape, row_steps (rows,)")
            a.p, a.state_sum, a.row_steps = p_.data_ptr(), s_.data_ptr(), st_.data_ptr()
            self._fill_rows(a, who, p_, i_, g_)
        return arr

    def rows_catch_up(self, tensors, counters, lr, weight_decay=1e-10, eps=1e-8):
        """okge_rows_catch_up: the rows the int32 device ids name take the decay-only steps they still owe, before anything
        reads them.  tensors: one or two (p, state_sum, ids, row_steps); counters: int32[2] on the device."""
        arr = self._rows_decay_tensors([(p, s, i, None, st) for p, s, i, st in tensors], "rows_catch_up")
        N.check(self.lib.okge_rows_catch_up(arr, len(tensors), counters.data_ptr(), float(lr), float(weight_decay), float(eps),
                                            self._stream()), "okge_rows_catch_up")

    def adagrad_rows_decay(self, tensors, counters, window, lr, weight_decay=1e-10, eps=1e-8):
        """okge_adagrad_rows_decay: okge_adagrad_rows with the dense step's weight-decay term on the named rows, then the due
        slice of the deferred decay-only steps and T += 1.  tensors: one or two (p, state_sum, ids, g, row_steps)."""
        arr = self._rows_decay_tensors(tensors, "adagrad_rows_decay")
        ws = self._rows_scratch(arr, self.lib.okge_adagrad_rows_workspace_bytes)
        N.check(self.lib.okge_adagrad_rows_decay(arr, len(tensors), counters.data_ptr(), int(window), float(lr), float(weight_decay),
                                                 float(eps), ws.data_ptr(), ws.numel(), self._stream()), "okge_adagrad_rows_decay")

    @staticmethod
    def lazy_tensors(tensors):
        """(p, g, state_sum[, row_steps, touched_map, stamp]) tuples -> the okge_lazy_tensor array of okge_adagrad_lazy"""
        arr = (N.LazyTensor * len(tensors))()
        for a, t in zip(arr, tensors):
            p, g, s = t[:3]
            a.p, a.g, a.state_sum = p.data_ptr(), g.data_ptr(), s.data_ptr()
            if len(t) > 3 and t[3] is not None:
                a.rows, a.row_len, a.row_steps = p.shape[0], p.shape[1], t[3].data_ptr()
                if len(t) > 4 and t[4] is not None:
                    a.row_touched, a.touched_stamp = t[4].data_ptr(), int(t[5])
            else:
                a.rows, a.row_len = 1, p.numel()
        return arr

    def adagrad_lazy(self, tensors, counters, window, flush, lr, weight_decay=1e-10, eps=1e-8):
        """okge_adagrad_lazy: the update with the weight-decay-only steps of rows no batch names deferred (flush=False: one
        optimizer step; flush=True: every row brought to the current step).  counters: int32[2] on the device."""
        arr = self.lazy_tensors(tensors)
        N.check(self.lib.okge_adagrad_lazy(arr, len(tensors), counters.data_ptr(), int(window), 1 if flush else 0, float(lr),
                                           float(weight_decay), float(eps), self._stream()), "okge_adagrad_lazy")

    def clip_grad_norm_(self, g0, g1, max_norm, norm_out=None):
        """torch.nn.utils.clip_grad_norm_ over two dense gradient tensors, in place (trainer.py:236-240)"""
        ws = self._side("_clip_ws", 8448)
        N.check(self.lib.okge_clip_grad_norm(g0.data_ptr(), g0.numel(), _ptr(g1), 0 if g1 is None else g1.numel(), float(max_norm),
                                             _ptr(norm_out), ws.data_ptr(), ws.numel(), self._stream()), "okge_clip_grad_norm")

    def merge_logsumexp(self, parts, out=None):
        """parts (world, B) fp32 per-shard row log-sum-exps -> (B,) log-sum-exp over the shards"""
        world, B = parts.shape
        if out is None:
            out = torch.empty(B, dtype=torch.float32, device=self.device)
        N.check(self.lib.okge_merge_logsumexp(parts.data_ptr(), world, B, out.data_ptr(), self._stream()), "okge_merge_logsumexp")
        return out

    def filtered_ranks(self, scores, filt_ptr, filt_col, row_ptr, grp_ptr, ids):
        """int64 ranks per answer group; all index arrays on the device (int64 ptr arrays, int32 ids)."""
        n_groups = int(grp_ptr.numel()) - 1
        ranks = torch.empty(n_groups, dtype=torch.int64, device=self.device)
        B, n = scores.shape
        N.check(self.lib.okge_filtered_ranks(scores.data_ptr(), scores.stride(0), B, n, filt_ptr.data_ptr(),
                                             _ptr(filt_col), row_ptr.data_ptr(), grp_ptr.data_ptr(), ids.data_ptr(),
                                             ranks.data_ptr(), self._stream()), "okge_filtered_ranks")
        return ranks

    def evaluate_batch(self, E, R, scorer, batch: PrefixBatch, filt_ptr, filt_col, row_ptr, grp_ptr, ids, scores, ranks,
                       acc, rank_stream, loss=None, label_smoothing=0.0):
        """score (current stream) -> filtered ranks -> meters (rank_stream) in one library call; `scores` (B, >=N) and
        `ranks` (>= n_groups int64) are caller buffers, `acc` 7 device doubles.  loss 'bce' / 'kl': also the batch's
        validation loss (okge_evaluate_batch_loss), returned as a one-element float64 device tensor written in rank_stream's
        order; None otherwise."""
        pb, c, keep = self._batch(batch)
        t = self._tables(E, R, scorer)
        n_groups = int(grp_ptr.numel()) - 1
        if loss is not None:
            need = int(self.lib.okge_evaluate_batch_loss_workspace_bytes(batch.B, t.d))
            if need == 0:
                raise N.OkgeError(f"invalid problem size B={batch.B} N={c.n} d={t.d}")
            ws = self._grow(need)
            out = torch.zeros(1, dtype=torch.float64, device=self.device)
            el = N.eval_loss(loss, label_smoothing, out.data_ptr())
            N.check(self.lib.okge_evaluate_batch_loss(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), filt_ptr.data_ptr(),
                                                      _ptr(filt_col), row_ptr.data_ptr(), grp_ptr.data_ptr(), ids.data_ptr(),
                                                      n_groups, scores.data_ptr(), scores.stride(0), ranks.data_ptr(),
                                                      acc.data_ptr(), ws.data_ptr(), self._ws_bytes, self._stream(),
                                                      ctypes.c_void_p(rank_stream.cuda_stream), ctypes.byref(el)),
                    "okge_evaluate_batch_loss")
            del keep
            return out
        ws = self.workspace(batch.B, c.n, t.d, "score")
        N.check(self.lib.okge_evaluate_batch(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), filt_ptr.data_ptr(),
                                             _ptr(filt_col), row_ptr.data_ptr(), grp_ptr.data_ptr(), ids.data_ptr(),
                                             n_groups, scores.data_ptr(), scores.stride(0), ranks.data_ptr(),
                                             acc.data_ptr(), ws.data_ptr(), self._ws_bytes, self._stream(),
                                             ctypes.c_void_p(rank_stream.cuda_stream)), "okge_evaluate_batch")
        del keep

    def evaluate_fused(self, E, R, scorer, batch: PrefixBatch, filt_ptr, filt_col, row_ptr, grp_ptr, ids, ranks=None, acc=None,
                       loss=None, label_smoothing=0.0):
        """filtered ranks + meters of one evaluation batch without the (B, N) score block (okge_evaluate_fused): ranks
        (int64 per answer group, bit-equal to score() + filtered_ranks()) and acc (7 device doubles, accumulated).
        loss 'bce' / 'kl': the same sweep also yields the batch's validation loss (okge_evaluate_fused_loss; the sum over the
        (B, N) elements, not divided) -> (ranks, acc, loss) with loss a one-element float64 device tensor."""
        pb, c, keep = self._batch(batch)
        t = self._tables(E, R, scorer)
        n_groups, n_filter = int(grp_ptr.numel()) - 1, int(filt_col.numel())
        size = self.lib.okge_eval_workspace_bytes if loss is None else self.lib.okge_eval_loss_workspace_bytes
        need = int(size(batch.B, c.n, t.d, n_groups, n_filter))
        self._grow(need)
        if ranks is None:
            ranks = torch.empty(max(n_groups, 1), dtype=torch.int64, device=self.device)
        if acc is None:
            acc = torch.zeros(7, dtype=torch.float64, device=self.device)
        if loss is not None:
            out = torch.zeros(1, dtype=torch.float64, device=self.device)
            el = N.eval_loss(loss, label_smoothing, out.data_ptr())
            N.check(self.lib.okge_evaluate_fused_loss(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), filt_ptr.data_ptr(),
                                                      _ptr(filt_col) if n_filter else None, n_filter, row_ptr.data_ptr(),
                                                      grp_ptr.data_ptr(), _ptr(ids), n_groups, ranks.data_ptr(), acc.data_ptr(),
                                                      self._ws.data_ptr(), self._ws_bytes, self._stream(), ctypes.byref(el)),
                    "okge_evaluate_fused_loss")
            del keep
            return ranks[:n_groups], acc, out
        N.check(self.lib.okge_evaluate_fused(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), filt_ptr.data_ptr(),
                                             _ptr(filt_col) if n_filter else None, n_filter, row_ptr.data_ptr(),
                                             grp_ptr.data_ptr(), ids.data_ptr(), n_groups, ranks.data_ptr(), acc.data_ptr(),
                                             self._ws.data_ptr(), self._ws_bytes, self._stream()), "okge_evaluate_fused")
        del keep
        return ranks[:n_groups], acc

    def evaluate_fused_shard(self, phase, E_local, R, scorer, Q, B, batch: PrefixBatch, shard: "Shard", n_cand_global, filt_ptr,
                             filt_col, row_ptr, grp_ptr, ids, true_scores, counts):
        """one launch of the candidate-sharded fused evaluation (okge_evaluate_fused_shard): phase 1 point scores ->
        true_scores (local maxima), 2 tile sweep, 4 counts; `batch` carries the LOCAL candidate range / list"""
        c = N.Candidates()
        cid = _i32(batch.cand_ids, self.device)
        c.ids, c.first_id, c.n = _ptr(cid), int(batch.cand_first), int(batch.n_candidates)
        t = self._tables(E_local, R, scorer)
        n_groups, n_filter = int(grp_ptr.numel()) - 1, int(filt_col.numel())
        need = int(self.lib.okge_eval_workspace_bytes(B, c.n, t.d, n_groups, n_filter))
        ews = self._side("_ews", need) if phase == 1 else self._ews                    # lives across the three phases
        sh = shard.c()
        N.check(self.lib.okge_evaluate_fused_shard(int(phase), ctypes.byref(t), ctypes.byref(sh), Q.data_ptr(), Q.stride(0), int(B),
                                                   ctypes.byref(c), int(n_cand_global), filt_ptr.data_ptr(),
                                                   _ptr(filt_col) if n_filter else None, n_filter, row_ptr.data_ptr(),
                                                   grp_ptr.data_ptr(), _ptr(ids), n_groups, true_scores.data_ptr(),
                                                   counts.data_ptr(), ews.data_ptr(), ews.numel(), self._stream()),
                "okge_evaluate_fused_shard")
        del cid

    def rank_metrics(self, ranks, acc):
        """acc (7 device doubles) += {n, sum 1/(r+1), sum r, #r<1, #r<3, #r<10, #r<50}"""
        N.check(self.lib.okge_rank_metrics(ranks.data_ptr(), int(ranks.numel()), acc.data_ptr(), self._stream()),
                "okge_rank_metrics")

    def group_true_scores(self, scores, col0, row_ptr, grp_ptr, ids):
        """float32 per answer group: max score over the group's ids inside columns [col0, col0 + n_local)."""
        out = torch.empty(int(grp_ptr.numel()) - 1, dtype=torch.float32, device=self.device)
        B, n = scores.shape
        N.check(self.lib.okge_group_true_scores(scores.data_ptr(), scores.stride(0), B, int(col0), n, row_ptr.data_ptr(),
                                                grp_ptr.data_ptr(), ids.data_ptr(), out.data_ptr(), self._stream()),
                "okge_group_true_scores")
        return out

    def rank_counts(self, scores, col0, filt_ptr, filt_col, row_ptr, true_scores):
        """int64 (n_groups, 2): {#greater, #equal} over the local candidate columns."""
        out = torch.empty((int(true_scores.numel()), 2), dtype=torch.int64, device=self.device)
        B, n = scores.shape
        N.check(self.lib.okge_rank_counts(scores.data_ptr(), scores.stride(0), B, int(col0), n, filt_ptr.data_ptr(),
                                          _ptr(filt_col), row_ptr.data_ptr(), true_scores.data_ptr(), out.data_ptr(),
                                          self._stream()), "okge_rank_counts")
        return out

    # -- measurement --------------------------------------------------------------------------------
    def timing(self, on):
        self.lib.okge_timing_enable(1 if on else 0)
        self.lib.okge_timing_reset()

    def timing_collect(self):
        return N.timing_collect()


def positives_from_dense(labels: torch.Tensor):
    """(B, N) {0,1} label matrix (what the reference's collate builds, dataset.py:885-932) -> coordinates
    sorted by column.  Container plumbing for the API-compatible entry points; the fused path consumes
    coordinates directly."""
    idx = labels.t().nonzero()               # sorted by (col, row)
    return idx[:, 1].to(torch.int32).contiguous(), idx[:, 0].to(torch.int32).contiguous()
