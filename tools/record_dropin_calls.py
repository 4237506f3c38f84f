#!/usr/bin/env python3
"""What AddLossModule asks of the library for the plain lookup models, call for call, on the CPU: every configuration of CONFIGS
runs the module on CPU tensors with the model's engine replaced by a HotPath that was made without its constructor (device cpu,
stream 0) and whose `lib` is a recorder.  Whatever route the module takes -- HotPath.forward_backward, PrefixCall.train on
persistent or on fresh structs -- ends in the same three entry points, okge_train_forward_backward, okge_n3_forward_backward and
okge_rescale_gradients, and the recorder decodes their ctypes arguments: every scalar, the flags word, the struct fields (counts,
first_id, the five dropout blocks) and, for every pointer, the NAME of the tensor it points to ("E", "g_e", "scores", "po_rel",
...; by data_ptr(), for converted id tensors by their contents; never the pointer value).  The recorder writes the number of the
call into loss_out (+ 0.5 into reg_out), so the returned loss shows which buffer the result was read from.  Per call of the
module the trace also holds m.dropout_step, shape and stride of all_outputs, shape / dtype / fill of the gradient buffers (torch's
uninitialised constructors are made to fill NaN while the module runs: "uninitialised" is by construction, not by luck), the
occurrence ids, the autograd Function that wrapped the result, whether autograd's multithreading was left on, and after
backward() what the two .grad are.

tests/test_dropin_calls.py compares the tree it runs in with tests/golden/dropin_calls.json, exactly, with FAST_CALL on AND off
against the same trace.  The fixture is what the commit BEFORE a change to trainer.py records with FAST_CALL on -- check that
commit out somewhere and

    python tools/record_dropin_calls.py --tree THAT_CHECKOUT --out tests/golden/dropin_calls.json

(--tree: the directory the package is imported from; default: this one).  Where that commit's own two routes differ, the file
therefore pins the fast route's value for both, and the recording prints every such place: at 0e3fb49 it is one, the flags word
of the sparse_grads call (OKGE_TRAIN_ROW_GRADS alone on the fast route, | OKGE_TRAIN_GRADS_ZERO on the general one; the library
ignores the difference).  One difference of that commit's routes is pinned the other way round: only its general route asked a
model that replaces dropout_spec for its masks (tests replay the reference's that way), so "replayed_masks" is recorded on dense
labels, which took the general route with the switch on and off."""
import argparse
import contextlib
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ENT, N_REL, D, FIRST = 50, 12, 16, 2
WORKSPACE_BYTES = 4096

# the four batches of tests/test_dropin_path.py (_STEP_SHAPES): po = (rel, obj), sp = (subj, rel), candidate id list or None for
# the 1-vs-all range, positives (row, col) sorted by col
SHAPES = [
    (([2, 3, 4], [5, 6, 7]), ([8, 9, 10, 11], [5, 6, 7, 8]), None, ([0, 3, 6, 2, 1, 5, 4], [1, 4, 9, 20, 33, 40, 47])),
    (None, ([12, 13, 14], [2, 3, 4]), [4, 9, 17, 30, 41, 22, 3], ([0, 1, 1, 2], [0, 2, 4, 6])),
    (([9, 10], [20, 21]), None, None, ([1], [7])),
    (([6], [22]), ([23, 24], [7, 8]), None, ([0, 2, 1], [3, 5, 30])),
]

# module keywords (loss, smoothing, training_outputs, sparse_grads, fused_l2_reg), model keywords (l2_reg), and how the run goes:
#   candidates  "list" (the batch's id list with use_batch_shared_entities, None for a range batch), "all_lists" (a list for every
#               batch, with use_batch_shared_entities), "whole_range" (the list of every entity, without), "none"
#   labels "coords" / "dense";  ids int32 / int64;  freeze: the tables without requires_grad;  modes: per batch "train" / "eval"
#   replayed_masks: m.dropout_spec is replaced by one that hands out `keep` masks (dense labels: at 0e3fb49 only the general
#               route asked the model, and dense labels took it with the switch on and off)
CONFIGS = {
    "bce": dict(),
    "bce_no_outputs": dict(training_outputs=False),
    "kl": dict(loss="kl", smoothing=0.1),
    "bce_smoothing": dict(smoothing=0.1),
    "id_lists": dict(candidates="all_lists"),
    "whole_range_list": dict(candidates="whole_range"),
    "dense_labels": dict(labels="dense"),
    "int64_ids": dict(ids="int64"),
    "sparse": dict(sparse_grads=True),
    "l2_reg_shared": dict(fused_l2_reg=True, l2_reg=0.05, candidates="all_lists"),
    "l2_reg_none": dict(fused_l2_reg=True, l2_reg=0.05, candidates="none"),
    "sparse_l2_reg": dict(sparse_grads=True, fused_l2_reg=True, l2_reg=0.05),
    "freeze_entities": dict(freeze=("entity",)),
    "freeze_relations": dict(freeze=("relation",), training_outputs=False),
    "freeze_both": dict(freeze=("entity", "relation")),
    "freeze_entities_sparse": dict(freeze=("entity",), sparse_grads=True),
    "freeze_relations_l2_reg": dict(freeze=("relation",), fused_l2_reg=True, l2_reg=0.05),
    "eval_no_grad": dict(modes=("eval",) * 4),
    "train_no_grad_l2_reg": dict(modes=("train_no_grad",) * 2, fused_l2_reg=True, l2_reg=0.05),
    "train_eval_sequence": dict(modes=("train", "eval", "train", "eval")),
    "validate": dict(validate=True, modes=("train", "unsorted", "eval")),
    "bad_tables": dict(bad_tables=True, modes=("train",)),
    "replayed_masks": dict(replayed_masks=True, labels="dense"),
}


class RecordingLib:
    """stands where the ctypes library stands: the three entry points are decoded and recorded, the workspace queries answer a
    constant, everything else is an error"""

    def __init__(self, engine):
        self.engine, self.calls, self.count, self.known, self.ids = engine, [], 0, {}, {}

    def name(self, ptr, n=None):
        """the name of the tensor at ptr: a tensor the run knows, else (n given: an id tensor) the input with these contents;
        a tensor made inside the module's call is named afterwards (resolve)"""
        ptr = getattr(ptr, "value", ptr)
        if not ptr:
            return "null"
        for name, t in self.known.items():
            if t is not None and t.data_ptr() == ptr:
                return name
        if n is not None:
            held = list((ctypes.c_int32 * n).from_address(ptr))
            same = [name for name, values in self.ids.items() if values == held]
            return same[0] if len(same) == 1 else "ids?"
        return {"ptr": ptr}

    def resolve(self, x, made):
        if isinstance(x, dict) and set(x) == {"ptr"}:
            return next((name for name, ptr in made.items() if ptr == x["ptr"]), "unknown")
        if isinstance(x, dict):
            return {k: self.resolve(v, made) for k, v in x.items()}
        return [self.resolve(v, made) for v in x] if isinstance(x, list) else x

    def take(self, made):
        out, self.calls = self.resolve(self.calls, made), []
        return out

    def _dropout(self, d):
        return [float(d.p), int(d.seed), int(d.stream), int(d.step), self.name(d.keep), self.name(d.step_dev)]

    def _structs(self, t, pb, c):
        t, pb, c = t._obj, pb._obj, c._obj
        return {"tables": {"E": self.name(t.E), "R": self.name(t.R), "n_ent": t.n_ent, "n_rel": t.n_rel, "d": t.d, "scorer": t.scorer},
                "batch": {"po_rel": self.name(pb.po_rel, pb.n_po), "po_obj": self.name(pb.po_obj, pb.n_po),
                          "sp_subj": self.name(pb.sp_subj, pb.n_sp), "sp_rel": self.name(pb.sp_rel, pb.n_sp), "n_po": pb.n_po, "n_sp": pb.n_sp},
                "cand": {"ids": self.name(c.ids, c.n), "first_id": c.first_id, "n": c.n, "table": self.name(c.table), "table_rows": c.table_rows},
                "dropout": [self._dropout(d) for d in (c.drop, pb.drop_po_ent, pb.drop_po_rel, pb.drop_sp_ent, pb.drop_sp_rel)]}

    def _ws(self, ws, ws_bytes):
        return ["ws" if self.engine._ws is not None and self.engine._ws.data_ptr() == ws else "not the workspace", int(ws_bytes)]

    def okge_train_forward_backward(self, t, pb, c, pos, loss, smoothing, normalizer, flags, loss_out, dE, dR, scores, ld, ws, ws_bytes, stream):
        self.count += 1
        ctypes.c_double.from_address(loss_out).value = float(self.count)
        pos = pos._obj
        self.calls.append({"call": "okge_train_forward_backward", **self._structs(t, pb, c),
                           "pos": {"row": self.name(pos.row, pos.nnz), "col": self.name(pos.col, pos.nnz), "nnz": pos.nnz},
                           "loss": int(loss), "label_smoothing": float(smoothing), "normalizer": float(normalizer), "flags": int(flags),
                           "dE": self.name(dE), "dR": self.name(dR), "scores": self.name(scores), "ld": int(ld),
                           "ws": self._ws(ws, ws_bytes), "stream": int(getattr(stream, "value", stream) or 0)})
        return 0

    def okge_n3_forward_backward(self, t, pb, c, coef, passes, normalizer, flags, reg_out, dE, dR, ws, ws_bytes, stream):
        ctypes.c_double.from_address(reg_out).value = float(self.count) + 0.5
        self.calls.append({"call": "okge_n3_forward_backward", **self._structs(t, pb, c), "coef": float(coef), "cand_passes": int(passes),
                           "normalizer": float(normalizer), "flags": int(flags), "dE": self.name(dE), "dR": self.name(dR),
                           "ws": self._ws(ws, ws_bytes), "stream": int(getattr(stream, "value", stream) or 0)})
        return 0

    def okge_rescale_gradients(self, g0, n0, g1, n1, alpha, applied, stream):
        self.calls.append({"call": "okge_rescale_gradients", "g0": self.name(g0), "n0": int(n0), "g1": self.name(g1), "n1": int(n1),
                           "alpha": float(ctypes.c_float.from_address(alpha).value), "applied": float(applied),
                           "stream": int(getattr(stream, "value", stream) or 0)})
        return 0

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *a: WORKSPACE_BYTES
        raise AttributeError(f"the recording library does not know {name!r}")


@contextlib.contextmanager
def poisoned_empty():
    """torch.empty / torch.empty_like / Tensor.new_empty fill floating tensors with NaN: a buffer that was not cleared shows"""
    import torch
    plain = torch.empty, torch.empty_like

    def poison(make):
        def made(*a, **kw):
            t = make(*a, **kw)
            return t.fill_(float("nan")) if t.is_floating_point() else t
        return made
    torch.empty, torch.empty_like = poison(torch.empty), poison(torch.empty_like)
    torch.Tensor.new_empty = poison(torch._C.TensorBase.new_empty)
    try:
        yield
    finally:
        torch.empty, torch.empty_like = plain
        del torch.Tensor.new_empty


def _engine():
    import torch
    from open_knowledge_graph_embeddings_amd import hotpath as H
    eng = H.HotPath.__new__(H.HotPath)
    eng.device, eng._ws, eng._ws_bytes = torch.device("cpu"), None, 0
    eng._stream = lambda: 0
    eng.lib = RecordingLib(eng)
    return eng


def _buffer(g):
    if g is None:
        return None
    fill = "uninitialised" if bool(g.isnan().all()) else "zero" if bool((g == 0).all()) else "other"
    return [list(g.shape), str(g.dtype), fill]


def _grad(p, made):
    g = p.grad
    if g is None:
        return None
    values = g._values() if g.is_sparse else g
    buffer = next((name for name, ptr in made.items() if ptr == values.data_ptr()), "a copy")
    return ["sparse" if g.is_sparse else "dense", list(g.shape), list(values.shape), buffer,
            g._indices().reshape(-1).tolist() if g.is_sparse else None]


def record_one(name, fast):
    """-> (the trace of configuration `name` with FAST_CALL = fast, whether the module made persistent structs)"""
    import torch
    from open_knowledge_graph_embeddings_amd import hotpath as H, trainer as T
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.model import Models
    kw = dict(CONFIGS[name])
    torch.manual_seed(1)
    m = Models.LookupComplexRelationModel(entity_slot_size=D, input_dropout=0.3, dropout=0.2 if kw.get("l2_reg") else 0.0,
                                          relation_input_dropout=0.1, init_std=0.1, sparse=False, l2_reg=kw.get("l2_reg", 0), seed=7,
                                          train_data=EntityRelationDatasetMeta(entities_size=N_ENT, relations_size=N_REL))
    if kw.get("bad_tables"):
        m.entity_embedding.weight.data = torch.zeros(D, N_ENT).t()
    for which in kw.get("freeze", ()):
        getattr(m, which + "_embedding").weight.requires_grad_(False)
    keeps = {}
    if kw.get("replayed_masks"):                       # the entity streams' masks come from the model, not from Philox
        keeps = {"keep_cand": (H.STREAM_CAND, torch.ones(N_ENT, D, dtype=torch.uint8)), "keep_po_ent": (H.STREAM_PO_ENT, torch.ones(4, D, dtype=torch.uint8)),
                 "keep_sp_ent": (H.STREAM_SP_ENT, torch.ones(4, D, dtype=torch.uint8))}
        by_stream = {stream: keep for stream, keep in keeps.values()}
        m.dropout_spec = lambda stream, relation=False: H.DropoutSpec(p=0.25, keep=by_stream[stream]) if stream in by_stream else H.DropoutSpec()
    eng = m._engine = _engine()
    lib = eng.lib
    loss = torch.nn.KLDivLoss(reduction="sum") if kw.get("loss") == "kl" else torch.nn.BCEWithLogitsLoss(reduction="sum")
    mod = T.AddLossModule(m, loss, kw.get("smoothing", 0.0), training_outputs=kw.get("training_outputs", True),
                          sparse_grads=kw.get("sparse_grads", False), fused_l2_reg=kw.get("fused_l2_reg", False))
    dt = torch.int64 if kw.get("ids") == "int64" else torch.int32
    ids = lambda x: None if x is None else torch.tensor(x, dtype=dt)                           # noqa: E731
    weights = m.entity_embedding.weight, m.relation_embedding.weight
    modes, trace = kw.get("modes", ("train",) * 4), []
    saved = T.FAST_CALL, H.VALIDATE
    T.FAST_CALL, H.VALIDATE = fast, bool(kw.get("validate"))
    try:
        for (po, sp, cand, pos), mode in zip(SHAPES, modes):
            candidates = kw.get("candidates", "list")
            use = candidates == "all_lists" or (candidates == "list" and cand is not None)
            if candidates == "whole_range":
                cand = list(range(FIRST, N_ENT))
            elif candidates == "all_lists" and cand is None:
                cand = list(range(N_ENT - 1, FIRST - 1, -1))
            elif candidates == "none":
                cand = None
            if mode == "unsorted":
                pos = (pos[0][::-1], pos[1][::-1])
            given = dict(po_rel=po and po[0], po_obj=po and po[1], sp_subj=sp and sp[0], sp_rel=sp and sp[1], cand_ids=cand,
                         pos_row=pos[0], pos_col=pos[1])
            tensors = {k: ids(v) for k, v in given.items()}
            if cand is not None:
                tensors["cand_ids"] = tensors["cand_ids"].reshape(-1, 1)                          # (as the collator hands it over)
            n = len(cand) if cand is not None else N_ENT - FIRST
            labels = (tensors["pos_row"], tensors["pos_col"])
            if kw.get("labels") == "dense":
                labels = torch.zeros((len(po[0] if po else ()) + len(sp[0] if sp else ()), n))
                labels[pos[0], pos[1]] = 1.0
            lib.known = {"E": m.E, "R": m.R, **tensors, **{k: keep for k, (_, keep) in keeps.items()}}
            lib.ids = {k: v for k, v in given.items() if v is not None}
            inputs = [po and (tensors["po_rel"], tensors["po_obj"]), sp and (tensors["sp_subj"], tensors["sp_rel"])]
            m.train(mode != "eval")
            m.zero_grad(set_to_none=True)
            torch.autograd.set_multithreading_enabled(True)
            step = {"mode": mode}
            try:
                with poisoned_empty(), torch.set_grad_enabled(mode not in ("eval", "train_no_grad")):
                    result, hook, outs = mod(inputs=inputs, labels=labels, use_batch_shared_entities=use, batch_shared_entities=tensors["cand_ids"],
                                             epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
            except (ValueError, H.N.OkgeError) as e:
                step.update(error=type(e).__name__, dropout_step=m.dropout_step, lib=lib.take({}))
                trace.append(step)
                continue
            fn = result.grad_fn
            g_e, g_r, rows = getattr(fn, "g_e", None), getattr(fn, "g_r", None), getattr(fn, "row_ids", None)
            # (by address, not by reference: a buffer nobody else holds is TAKEN as .grad, not copied)
            made = {k: t.data_ptr() for k, t in (("scores", outs), ("g_e", g_e), ("g_r", g_r)) if t is not None}
            step.update(lib=lib.take(made), dropout_step=m.dropout_step, result=float(result.detach()),
                        hook=None if hook is None else float(hook.detach()),
                        outputs=None if outs is None else [list(outs.shape), list(outs.stride())],
                        wrapped=None if fn is None else type(fn).__name__, hook_wrapped=None if hook is None or hook.grad_fn is None else hook.grad_fn is fn,
                        g_e=_buffer(g_e), g_r=_buffer(g_r), row_ids=None if rows is None else [r.tolist() for r in rows],
                        multithreading=torch.autograd.is_multithreading_enabled())
            wanted, g_e, g_r, rows, fn = fn is not None, None, None, None, None
            if wanted:
                ((result.sum() if hook is None else result.sum() + hook) / float(labels[0].numel() if isinstance(labels, tuple) else labels.numel())).backward()
                step["backward"] = {"lib": lib.take(made), "grad_e": _grad(weights[0], made), "grad_r": _grad(weights[1], made)}
            trace.append(step)
    finally:
        T.FAST_CALL, H.VALIDATE = saved
        torch.autograd.set_multithreading_enabled(True)
    return trace, getattr(mod, "_fd", None) is not None


def _differences(a, b, where=""):
    if isinstance(a, dict) and isinstance(b, dict) and set(a) == set(b):
        return [d for k in a for d in _differences(a[k], b[k], f"{where}.{k}")]
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in _differences(x, y, f"{where}[{i}]")]
    return [] if a == b else [f"{where}: {a!r} (fast) != {b!r} (general)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="import the package from this checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "dropin_calls.json"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import open_knowledge_graph_embeddings_amd.trainer as T
    assert os.path.abspath(T.__file__).startswith(os.path.abspath(args.tree) + os.sep), T.__file__
    golden = {}
    for name in CONFIGS:
        golden[name] = json.loads(json.dumps(record_one(name, True)[0]))
        for d in _differences(golden[name], json.loads(json.dumps(record_one(name, False)[0])), name):
            print("the two routes differ, the fast route's value is kept --", d)
    with open(args.out, "w") as f:
        json.dump(golden, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, "from", T.__file__)


if __name__ == "__main__":
    main()
