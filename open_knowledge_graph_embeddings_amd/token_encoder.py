"""What the token encoders on the virtual-table step (lstm.py, bigram.py) have in common: the pass driver over the native
calls, the step hooks between virtual_tables.VirtualTableStep and the two train steps, the encode autograd.Function and the
embedder plumbing.  An encoder module brings its slot class, the marshalling of its two native calls, its optimizer step and
its torch modules; a slot says what the shared code needs to know about it:

    what           "LSTM" / "bigram", for messages                pass_class   its EncoderPass subclass
    has_raw        encode takes a raw buffer in front of out      encoder_grads()   -> (the argument backward() takes for
                   (rows before the batch-norm)                                        the encoder's gradients, the same as a list)
"""
from __future__ import annotations

import ctypes

import torch

from . import _native as N
from . import hotpath as H
from . import virtual_tables as VT
from .token_embedder import TokenBasedRelationEmbedder

MAX_SLOT = 512                                     # the fused tile kernels' largest slot size
PRECOMPUTE_CHUNK = 16384                           # rows per encode call of precompute_embeddings_from_tokens


class EncoderPass:
    """The workspace of one pass (a slot's calls of one step) and the ctypes driver of its two native calls.  A backward
    needs the workspace its forward left: one object per pass in flight.  A subclass names the calls (`what`,
    `workspace_bytes`) and marshals their arguments in encode() / backward()."""

    what = workspace_bytes = None

    def __init__(self, device):
        self.device = torch.device(device)
        self.lib = N.lib()
        self.ws, self.ws_bytes = None, 0
        self.pos_tok = None
        self.rows, self.trained = 0, False

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _calls(self, calls):
        arr = (N.TokenCall * len(calls))()
        for x, (ids, first_id, n) in zip(arr, calls):
            x.ids, x.first_id, x.n = None if ids is None else ids.data_ptr(), int(first_id), int(n)
        return arr

    def _native(self, fn, slot, calls, *args):
        """fn(slot, calls, n_calls, *args, workspace, workspace_bytes, stream): the shape of both native calls"""
        s = slot.c()
        N.check(getattr(self.lib, fn)(ctypes.byref(s), self._calls(calls), len(calls), *args,
                                      0 if self.ws is None else self.ws.data_ptr(), self.ws_bytes, self._stream()), fn)

    def _encode(self, fn, slot, calls, training, *args):
        """grow the workspace and pos_tok to the pass, run the native encode (args: between `training` and pos_tok); a
        backward is allowed only once a training-mode encode has returned"""
        rows = sum(int(c[2]) for c in calls)
        need = int(getattr(self.lib, self.workspace_bytes)(rows, slot.L, slot.d, int(bool(training))))
        if need > self.ws_bytes:
            self.ws, self.ws_bytes = torch.empty(need, dtype=torch.uint8, device=self.device), need
        if self.pos_tok is None or self.pos_tok.numel() < rows * slot.L:
            self.pos_tok = torch.empty(max(rows * slot.L, 1), dtype=torch.int32, device=self.device)
        self.rows, self.trained = rows, False
        self._native(fn, slot, calls, int(bool(training)), *args, self.pos_tok.data_ptr())
        self.trained = bool(training)

    def _sorted_positions(self, slot):
        """-> the pass's pos_tok and its stable argsort, as pointers' owners (index plumbing; the sums are the kernel's)"""
        if not self.trained:
            raise RuntimeError(f"{self.what} backward without a training-mode forward")
        pos = self.pos_tok[:self.rows * slot.L]
        return pos, torch.argsort(pos, stable=True).to(torch.int32)


def bn_grad_pointers(slot, d_bn):
    """(d weight, d bias) halves of d_bn ([w | b]) as the native calls take them; None without a batch-norm"""
    if slot.bn is None:
        return None, None
    return d_bn[:slot.d].data_ptr(), d_bn[slot.d:].data_ptr()


class EncoderTrainStep(VT.VirtualTableStep):
    """VirtualTableStep with one EncoderPass per slot: the three entity calls share one pass and the two relation calls
    another, in the reference's encode order (trainer.py:75-91).  The optimizer is dense (no deferred updates).  A subclass
    brings _encode_slot, _backward_slot, _bn_state and optimizer_step."""

    def __init__(self, entity, relation, scorer, *args, **kwargs):
        super().__init__(entity, relation, scorer, *args, **kwargs)
        self.passes = (entity.pass_class(self.device), entity.pass_class(self.device))
        self.decay_window = 1

    def state_tensors(self):
        out = []
        for sl in (self.entity, self.relation):
            out += [sl.W, sl.dW, sl.sumW, sl.flat, sl.d_flat, sl.sum_flat]
            if sl.bn is not None:
                out += self._bn_state(sl)
        return out + self._optimizer_state()

    def _param_groups(self, every=False):
        """the slots' optimizer_tensors(); every=False: without those of a slot the scorer leaves unused"""
        return [t for sl in (self.entity, self.relation) if every or not self._unused(sl) for t in sl.optimizer_tensors()]

    def flush(self):
        """(no deferred updates here: every parameter is current after every step)"""

    def _encode(self, batch: H.PrefixBatch, bufs):
        """one pass per slot over its calls; -> the two slots' non-empty calls"""
        EV, EX, dEV, RV, RX, dRV = bufs
        calls = ([], [])
        for relation, ids, first, rows in VT.encode_calls(batch):
            if rows.stop > rows.start:
                calls[relation].append((H._i32(ids, self.device), first, rows.stop - rows.start))
        self._encode_slot(self.passes[0], self.entity, calls[0], EV, EX)
        self._encode_slot(self.passes[1], self.relation, calls[1], RV, RX)
        return calls

    def _backward(self, batch, bufs, calls):
        """dEV / dRV -> back through the encoder -> the slots' gradients"""
        EV, EX, dEV, RV, RX, dRV = bufs
        for ps, sl, cs, X, dV in zip(self.passes, (self.entity, self.relation), calls, (EX, RX), (dEV, dRV)):
            self._backward_slot(ps, sl, cs, X, dV)


class EncodeFn(torch.autograd.Function):
    """encode_* with gradients enabled (a caller's own loss): the HIP forward and backward of ONE call, with a workspace of
    its own (kept until backward).  Inputs after the first three are the slot's parameters, so that autograd hands their
    gradients on: W, the encoder's tensors[, bn weight, bn bias]."""

    @staticmethod
    def forward(ctx, ids, module, relation, W, *params):
        slot = module._slot(relation)
        n = ids.numel()
        out = torch.empty((n, slot.d), device=ids.device)
        raw = ((torch.empty_like(out) if slot.bn is not None else out),) if slot.has_raw else ()
        ps = slot.pass_class(ids.device)
        training = module.training
        ps.encode(slot, [(ids, 0, n)], training, *raw, out)
        ctx.slot, ctx.ps, ctx.ids, ctx.raw, ctx.training = slot, ps, ids, raw, training
        return out

    @staticmethod
    def backward(ctx, g):
        slot = ctx.slot
        if not ctx.training:
            raise RuntimeError(f"gradients of an eval-mode {slot.what} encode are not implemented (the running statistics "
                               f"have no graph)")
        d = slot.d
        dW = torch.zeros_like(slot.W)
        grads, grad_list = slot.encoder_grads()
        d_bn = torch.empty(2 * d, device=g.device) if slot.bn is not None else None
        ctx.ps.backward(slot, [(ctx.ids, 0, ctx.ids.numel())], *ctx.raw, g.contiguous(), dW, grads, d_bn)
        bn_grads = () if d_bn is None else (d_bn[:d].clone(), d_bn[d:].clone())
        return (None, None, None, dW, *grad_list, *bn_grads)


class TokenEncoderEmbedder(TokenBasedRelationEmbedder):
    """A token embedder whose rows come from an EncoderPass: _encode, the chunked precompute.  A subclass brings the
    constructor (through _refuse_unsupported, _init_token_tables and _init_state), _parts(relation), _params(relation),
    _slot(relation) -> a slot over the module's current parameters without gradient buffers, _precompute_chunk() -> its
    module's PRECOMPUTE_CHUNK, and what the base class asks of every token embedder for the training bridges."""

    max_slot = MAX_SLOT

    def _encode(self, ids, relation, stream):
        """the encoder (batch statistics in training mode, running statistics otherwise) -> dropout"""
        eng = self.engine()
        ids = ids.reshape(-1).to(torch.int32).contiguous()
        n = ids.numel()
        p = (self.relation_dropout if relation else self.entity_dropout) if self.training else 0.0
        params = self._params(relation)
        if torch.is_grad_enabled() and any(q.requires_grad for q in params):
            from . import autograd_score as AG
            out = EncodeFn.apply(ids, self, relation, *params)
            if p > 0:
                out = AG.MaskRowsFn.apply(out, eng, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
            return out.unsqueeze(1)
        out = torch.empty((n, self.slot_size), device=ids.device)
        if n:
            self._encode_rows(self._slot(relation), None, [(ids, 0, n)], self.training, out)
        if p > 0:
            out = eng.encode_rows(out, None, 0, n, H.DropoutSpec(p, self.dropout_seed, stream, self.dropout_step))
        return out.unsqueeze(1)

    @staticmethod
    def _encode_rows(slot, ps, calls, training, out):
        """one pass without a backward to follow: the raw rows, where the encoder has them, go to a scratch buffer"""
        raw = ((torch.empty_like(out) if slot.bn is not None else out),) if slot.has_raw else ()
        (ps or slot.pass_class(out.device)).encode(slot, calls, training, *raw, out)

    def precompute_embeddings_from_tokens(self):
        """model.py:670-712 (the reference encodes 4096 rows per call; in eval mode any chunk size gives the same rows)"""
        if self.entity_embedding_from_tokens is None:
            super().train(False)                       # the reference calls self.eval() here and stays in eval mode
            dev = self.entity_embedding.weight.device
            chunk = self._precompute_chunk()

            def table(n, relation):
                out = torch.empty((n, self.slot_size), device=dev)
                slot = self._slot(relation)
                ps = slot.pass_class(dev)
                for lo in range(0, n, chunk):
                    self._encode_rows(slot, ps, [(None, lo, min(chunk, n - lo))], False, out[lo:lo + chunk])
                return out
            with torch.no_grad():
                self.entity_embedding_from_tokens = table(self.train_data.entities_size, False)
                self.relations_embedding_from_tokens = table(self.train_data.relations_size, True)
