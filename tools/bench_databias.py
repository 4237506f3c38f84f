#!/usr/bin/env python3
"""Data-bias baseline models (DataBiasOnlyRelationModel / DataBiasOnlyEntityModel, openkge/model.py:281-350): one JSON line
with the HIP training step (lstm.LSTMTrainStep under the "bias_relation" / "bias_entity" scorer) beside LSTM-DistMult at the
same shape, and the reference's op sequence in torch-ROCm on the same GPU (nn.LSTM = MIOpen, ATen for the rest,
torch.optim.Adagrad, which skips the parameters without a gradient).

The shape is tools/bench_lstm.py's S-FB-lstm (d = 512, |E| = 14 543, B = 4096, 1-vs-all, batch-norm, dropout 0.1, max_len 10).
Every step is timed in `--windows` windows of `--steps` steps, the models taking turns window by window; the figures are the
windows' median with their lowest and highest beside it (the spread a difference has to clear).  The entity model skips the
relation slot's backward through time and its optimizer segments; the relation model is the ordinary step.
Usage: python tools/bench_databias.py [--steps K] [--warmup W] [--windows M] [--shape S-FB-lstm]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep  # noqa: E402
from open_knowledge_graph_embeddings_amd.synthetic import make_token_matrix  # noqa: E402
from bench_configs import positives_batch  # noqa: E402
from bench_lstm import SHAPES, make_slot  # noqa: E402

SCORERS = ("distmult", "bias_relation", "bias_entity")


def torch_reference_step(scorer, ent_tok, rel_tok, vt_e, vt_r, d, dev, dropout=0.1):
    """the reference's op sequence (model.py:966-986, :304-308 / :340-344, trainer.py:75-106, 221-244) in torch on the GPU: both
    prefix slots are encoded, one reaches the score"""
    emb_e = torch.nn.Embedding(vt_e, d, padding_idx=0).to(dev)
    emb_r = torch.nn.Embedding(vt_r, d, padding_idx=0).to(dev)
    bn_e, bn_r = torch.nn.BatchNorm1d(d).to(dev), torch.nn.BatchNorm1d(d).to(dev)
    lstm_e = torch.nn.LSTM(d, d, batch_first=True).to(dev)
    lstm_r = torch.nn.LSTM(d, d, batch_first=True).to(dev)
    params = [emb_e.weight, emb_r.weight, *bn_e.parameters(), *bn_r.parameters(), *lstm_e.parameters(), *lstm_r.parameters()]
    opt = torch.optim.Adagrad(params, lr=0.1, weight_decay=1e-10)
    te, tr = torch.from_numpy(ent_tok).to(dev).long(), torch.from_numpy(rel_tok).to(dev).long()

    def enc(ids, tok, emb, lstm, bn):
        x = tok[ids.long()]
        last = (x > 0).long().sum(1) - 1
        out, _ = lstm(emb(x))
        return torch.nn.functional.dropout(bn(out[torch.arange(x.shape[0], device=dev), last]), dropout, True)

    def step(batch, cand):
        opt.zero_grad(set_to_none=True)
        C = enc(cand, te, emb_e, lstm_e, bn_e)
        r_po, o = enc(batch.po_rel, tr, emb_r, lstm_r, bn_r), enc(batch.po_obj, te, emb_e, lstm_e, bn_e)
        s, r_sp = enc(batch.sp_subj, te, emb_e, lstm_e, bn_e), enc(batch.sp_rel, tr, emb_r, lstm_r, bn_r)
        q = torch.cat([r_po, r_sp]) if scorer == "bias_relation" else torch.cat([o, s])
        scores = q @ C.t()
        y = torch.zeros_like(scores)
        y[batch.pos_row.long(), batch.pos_col.long()] = 1.0
        loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, y, reduction="sum")
        (loss / scores.numel()).backward()
        opt.step()
    return step


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def summary(ws):
    return {"ms_per_step": round(float(np.median(ws)), 3), "min": round(min(ws), 3), "max": round(max(ws), 3),
            "windows": [round(w, 3) for w in ws]}


def measure(name, dev, steps, warmup, windows):
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    n_ent, n_rel, vt_e, vt_r, d, B, N, L = SHAPES[name]
    ent_tok, rel_tok = make_token_matrix(rng, n_ent, vt_e, L), make_token_matrix(rng, n_rel, vt_r, L)
    if N is None:
        batches = [positives_batch(rng, t, n_ent, n_rel, B, n_ent - 2, 2) for _ in range(2)]
        cand = [np.arange(2, n_ent)] * 2
    else:
        cand = [rng.choice(n_ent - 2, N, replace=False).astype(np.int32) + 2 for _ in range(2)]
        batches = [positives_batch(rng, t, n_ent, n_rel, B, N, 1, cand_ids=t(c)) for c in cand]
    fns = {}
    for scorer in SCORERS:
        st = LSTMTrainStep(make_slot(rng, dev, vt_e, ent_tok, d), make_slot(rng, dev, vt_r, rel_tok, d), scorer, lr=0.1, dropout=0.1,
                           seed=1)
        fns[scorer] = (lambda st=st, i=[0]: (st.step(batches[i[0] % 2]), i.__setitem__(0, i[0] + 1)))
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    times = {k: [] for k in fns}
    for _ in range(windows):                                    # the models take turns: drift hits them alike
        for k, fn in fns.items():
            times[k].append(window(fn, steps))
    res = {"shape": name, "d": d, "B": B, "N": N if N is not None else n_ent - 2, "max_len": L, "steps_per_window": steps,
           "hip": {k: summary(v) for k, v in times.items()}}
    fns.clear()
    torch.cuda.empty_cache()
    cand_t = [t(c.astype(np.int32)) for c in cand]
    res["torch_rocm"] = {}
    for scorer in SCORERS[1:]:
        try:
            ref = torch_reference_step(scorer, ent_tok, rel_tok, vt_e, vt_r, d, dev)
            j = [0]

            def ref_one():
                ref(batches[j[0] % 2], cand_t[j[0] % 2])
                j[0] += 1
            for _ in range(2):
                ref_one()
            res["torch_rocm"][scorer] = summary([window(ref_one, max(3, steps // 4)) for _ in range(3)])
            del ref
        except torch.cuda.OutOfMemoryError as e:
            res["torch_rocm"][scorer] = {"ms_per_step": None, "error": str(e).splitlines()[0]}
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--shape", default="S-FB-lstm")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({"metric": "data-bias baseline models, training step", "results": [measure(a.shape, dev, a.steps, a.warmup, a.windows)]}),
          flush=True)


if __name__ == "__main__":
    main()
