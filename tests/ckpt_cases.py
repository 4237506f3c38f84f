"""What the checkpoint tests (test_ckpt_layout / test_ckpt_resume / test_ckpt_reference) share: the five model kinds built from
the g22_ckpt_* fixtures (tests/golden/make_golden_ckpt.py), the fixtures' checkpoints as the dicts `Trainer.save` wrote, and the
flat (path, tensor) view of such a dict that the fixtures' key lists are written in."""
import json

import numpy as np
import torch

from conftest import golden

KINDS = ("unigram", "lstm", "bias_entity", "bigram", "tucker3")
OPTIMIZERS = ("adagrad", "adam")
P_DROP = 0.25


def fixture(kind):
    return golden("g22_ckpt_" + kind)


def build(kind, dropout=0.0, seed=None):
    """this package's module of `kind` on the CPU at the fixture's sizes and token maps; seed: every parameter redrawn from it"""
    z = fixture(kind)
    if kind == "tucker3":
        from test_tucker3_reference import construct
        m = construct(z, input_dropout=dropout, relation_input_dropout=dropout)
    elif kind == "bigram":
        from test_bigram_api import build as make
        m = make(z, dropout=dropout)
    else:
        from test_lstm_api import build as make
        m = make(z, dropout=dropout, **({"pool": "sum"} if kind == "unigram" else {}))
    if seed is not None:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    return m


def flat(ckpt):
    """[(path, tensor)] in the checkpoint's own order: "state_dict/<key>", then "optimizer/<param index>/<state key>" """
    out = [("state_dict/" + k, v) for k, v in ckpt["state_dict"].items()]
    for i, st in ckpt["optimizer_state_dict"][0]["optimizer_state"]["state"].items():
        out += [(f"optimizer/{i}/{k}", v) for k, v in st.items()]
    return out


def layout(pairs):
    return [(p, "x".join(str(n) for n in t.shape), str(t.dtype)) for p, t in pairs]


def fixture_layout(z, run=""):
    return list(zip((str(k) for k in z[run + "ckpt_keys"]), (str(s) for s in z[run + "ckpt_shapes"]), (str(t) for t in z[run + "ckpt_dtypes"])))


def fixture_checkpoint(z, run="", which="ckpt"):
    """the dict the reference held after two (`ckpt`) or three (`end`) steps, as torch.load would return it"""
    meta = json.loads(str(z[run + "ckpt_meta"]))
    sd, state = {}, {}
    for path in (str(k) for k in z[run + "ckpt_keys"]):
        t = torch.tensor(z[f"{run}{which}/{path}"])
        head, _, rest = path.partition("/")
        if head == "state_dict":
            sd[rest] = t
        else:
            i, _, name = rest.partition("/")
            state.setdefault(int(i), {})[name] = t
    return {"epoch": meta["epoch"], "training_steps": meta["training_steps"] + (which == "end"), "state_dict": sd,
            "optimizer_state_dict": [{"optimizer_state": {"state": state, "param_groups": meta["param_groups"]}, "regime": meta["regime"]}],
            "validation_results": None}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fixture_batch(z, s):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    pre = f"s{s}_"
    b = PrefixBatch(po_rel=dev(z[pre + "po_rel"].reshape(-1)), po_obj=dev(z[pre + "po_obj"].reshape(-1)),
                    sp_subj=dev(z[pre + "sp_subj"].reshape(-1)), sp_rel=dev(z[pre + "sp_rel"].reshape(-1)),
                    cand_ids=dev(z[pre + "cand"].reshape(-1).astype(np.int32)))
    b.pos_row, b.pos_col = positives_from_dense(dev(z[pre + "labels"]))
    return b


def random_batches(kind, pattern="alal", n_po=6, n_sp=5, seed=11):
    """batches over the fixture's ids; pattern: 'a' = 1-vs-all (the candidate range), 'l' = a list that names 24 candidates once"""
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    z = fixture(kind)
    n_ent, n_rel = int(z["n_ent"]), int(z["n_rel"])
    rng = np.random.default_rng(seed)
    out = []
    for what in pattern:
        ids = lambda hi, k: dev(rng.integers(2, hi, k).astype(np.int32))          # noqa: E731
        b = PrefixBatch(po_rel=ids(n_rel, n_po), po_obj=ids(n_ent, n_po), sp_subj=ids(n_ent, n_sp), sp_rel=ids(n_rel, n_sp))
        if what == "a":
            b.cand_first, b.n_cand = 2, n_ent - 2
        else:
            b.cand_ids, b.cand_unique = dev(rng.permutation(np.arange(2, n_ent))[:24].astype(np.int32)), True
        y = np.zeros((n_po + n_sp, b.n_candidates), np.float32)
        y[np.arange(n_po + n_sp), rng.integers(0, b.n_candidates, n_po + n_sp)] = 1
        b.pos_row, b.pos_col = positives_from_dense(dev(y))
        out.append(b)
    return out
