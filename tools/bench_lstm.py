#!/usr/bin/env python3
"""LSTM-encoded models: one JSON line with the HIP training step (lstm.LSTMTrainStep) at two shapes, beside the reference's op
sequence in torch-ROCm on the same GPU (nn.LSTM = MIOpen, ATen for the rest, torch.optim.Adagrad).

  S-FB-lstm   config/fb15k237/fb15k237-complex-lstm.yaml: ComplEx d=512, |E| = 14 543, B = 4096, 1-vs-all, batch-norm,
              dropout 0.1, max_len 10 (synthetic Zipf mention tokens)
  S-OLP-lstm  the S-OLP-tok shape with the LSTM: ComplEx d=512, 2.5 M entities with synthetic tokens
              (synthetic.make_token_matrix), B = 4096, batch-shared N = 4096, batch-norm, dropout 0.1

Per shape: step ms and triples/s; P (the (row, position) pairs the LSTM steps through, from the ids); LSTM FLOP per step
(16 P d^2 forward + 32 P d^2 backward); the LSTM calls' HIP-event time (okge_lstm_encode_calls + okge_lstm_backward_calls:
sort, steps, batch-norm, weight gradients, scatter) and the FLOP share of the fp32-MFMA peak in it; eval precompute entities/s;
the torch-ROCm step.  Usage: python tools/bench_lstm.py [--steps K] [--warmup W] [--shapes S-FB-lstm,S-OLP-lstm]
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

from open_knowledge_graph_embeddings_amd import hotpath as H  # noqa: E402
from open_knowledge_graph_embeddings_amd.lstm import LSTMSlot, LSTMTrainStep, LstmPass, PRECOMPUTE_CHUNK  # noqa: E402
from open_knowledge_graph_embeddings_amd.synthetic import make_token_matrix  # noqa: E402
from bench_configs import positives_batch  # noqa: E402

PEAK_TFLOPS = 157.3                  # fp32 MFMA, MI355X
SHAPES = {
    # n_ent, n_rel, vocab_e, vocab_r, d, B, N (None: 1-vs-all), max_len
    "S-FB-lstm": (14_543, 239, 30_000, 2_000, 512, 4096, None, 10),
    "S-OLP-lstm": (2_500_000, 100_000, 200_000, 50_000, 512, 4096, 4096, 10),
}


def live_positions(tok, ids):
    live = (tok[ids] > 0).sum(1)
    return int(np.where(live > 0, live, tok.shape[1]).sum())


def make_slot(rng, dev, vocab, tok, d):
    b = 1.0 / np.sqrt(d)
    lstm = [torch.empty((4 * d, d), device=dev).uniform_(-b, b), torch.empty((4 * d, d), device=dev).uniform_(-b, b),
            torch.empty(4 * d, device=dev).uniform_(-b, b), torch.empty(4 * d, device=dev).uniform_(-b, b)]
    flat = torch.cat([x.reshape(-1) for x in lstm])
    views, o = [], 0
    for x in lstm:
        views.append(flat[o:o + x.numel()].view_as(x))
        o += x.numel()
    return LSTMSlot(torch.randn((vocab, d), device=dev) * 0.1, torch.from_numpy(tok).to(dev), views,
                    (torch.rand(d, device=dev), torch.zeros(d, device=dev)), (torch.zeros(d, device=dev), torch.ones(d, device=dev)),
                    flat=flat)


def torch_reference_step(ent_tok, rel_tok, vt_e, vt_r, d, dev, dropout=0.1):
    """the reference's op sequence (model.py:966-986 + :198-229 + trainer.py:75-106, 221-244) in torch on the GPU"""
    emb_e = torch.nn.Embedding(vt_e, d, padding_idx=0).to(dev)
    emb_r = torch.nn.Embedding(vt_r, d, padding_idx=0).to(dev)
    bn_e, bn_r = torch.nn.BatchNorm1d(d).to(dev), torch.nn.BatchNorm1d(d).to(dev)
    lstm_e = torch.nn.LSTM(d, d, batch_first=True).to(dev)
    lstm_r = torch.nn.LSTM(d, d, batch_first=True).to(dev)
    params = [emb_e.weight, emb_r.weight, *bn_e.parameters(), *bn_r.parameters(), *lstm_e.parameters(), *lstm_r.parameters()]
    opt = torch.optim.Adagrad(params, lr=0.1, weight_decay=1e-10)
    te, tr = torch.from_numpy(ent_tok).to(dev).long(), torch.from_numpy(rel_tok).to(dev).long()
    h = d // 2

    def enc(ids, tok, emb, lstm, bn):
        x = tok[ids.long()]
        last = (x > 0).long().sum(1) - 1
        out, _ = lstm(emb(x))
        return torch.nn.functional.dropout(bn(out[torch.arange(x.shape[0], device=dev), last]), dropout, True)

    def step(batch, cand):
        opt.zero_grad()
        C = enc(cand, te, emb_e, lstm_e, bn_e)
        r_po, o = enc(batch.po_rel, tr, emb_r, lstm_r, bn_r), enc(batch.po_obj, te, emb_e, lstm_e, bn_e)
        s, r_sp = enc(batch.sp_subj, te, emb_e, lstm_e, bn_e), enc(batch.sp_rel, tr, emb_r, lstm_r, bn_r)
        q_po = torch.cat([o[:, :h] * r_po[:, :h] + o[:, h:] * r_po[:, h:], o[:, h:] * r_po[:, :h] - o[:, :h] * r_po[:, h:]], 1)
        q_sp = torch.cat([s[:, :h] * r_sp[:, :h] - s[:, h:] * r_sp[:, h:], s[:, h:] * r_sp[:, :h] + s[:, :h] * r_sp[:, h:]], 1)
        scores = torch.cat([q_po, q_sp]) @ C.t()
        y = torch.zeros_like(scores)
        y[batch.pos_row.long(), batch.pos_col.long()] = 1.0
        loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, y, reduction="sum")
        (loss / scores.numel()).backward()
        opt.step()
    return step


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def measure(name, dev, steps, warmup):
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    n_ent, n_rel, vt_e, vt_r, d, B, N, L = SHAPES[name]
    ent_tok, rel_tok = make_token_matrix(rng, n_ent, vt_e, L), make_token_matrix(rng, n_rel, vt_r, L)
    ent, rel = make_slot(rng, dev, vt_e, ent_tok, d), make_slot(rng, dev, vt_r, rel_tok, d)
    st = LSTMTrainStep(ent, rel, "complex", lr=0.1, dropout=0.1, seed=1)
    if N is None:
        batches = [positives_batch(rng, t, n_ent, n_rel, B, n_ent - 2, 2) for _ in range(2)]
        cand = [np.arange(2, n_ent)] * 2
    else:
        cids = [rng.choice(n_ent - 2, N, replace=False).astype(np.int32) + 2 for _ in range(2)]
        batches = [positives_batch(rng, t, n_ent, n_rel, B, N, 1, cand_ids=t(c)) for c in cids]
        cand = cids
    b0 = batches[0]
    ent_ids = np.concatenate([cand[0], b0.po_obj.cpu().numpy(), b0.sp_subj.cpu().numpy()])
    rel_ids = np.concatenate([b0.po_rel.cpu().numpy(), b0.sp_rel.cpu().numpy()])
    P_e, P_r = live_positions(ent_tok, ent_ids), live_positions(rel_tok, rel_ids)
    P = P_e + P_r
    lstm_flop = 48.0 * P * d * d
    i = [0]

    def one():
        st.step(batches[i[0] % 2])
        i[0] += 1
    ms = timed(one, steps, warmup)
    st.engine.timing(True)
    for _ in range(5):
        one()
    torch.cuda.synchronize()
    per = {k: v[0] / v[1] * 1e3 for k, v in st.engine.timing_collect().items()}
    st.engine.timing(False)
    lstm_us = 2 * (per.get("lstm_encode", 0.0) + per.get("lstm_backward", 0.0))           # two passes (entity, relation) per step
    # eval precompute: entity rows in PRECOMPUTE_CHUNK-row encode calls, running statistics
    n_eval = min(n_ent, 16 * PRECOMPUTE_CHUNK)
    ps, out = LstmPass(dev), torch.empty((PRECOMPUTE_CHUNK, d), device=dev)
    raw = torch.empty_like(out)

    def pre():
        for lo in range(0, n_eval, PRECOMPUTE_CHUNK):
            m = min(PRECOMPUTE_CHUNK, n_eval - lo)
            ps.encode(ent, [(None, lo, m)], False, raw[:m], out[:m])
    pre_ms = timed(pre, 3, 1)
    res = {"shape": name, "d": d, "B": B, "N": N if N is not None else n_ent - 2, "max_len": L,
           "ms_per_step": round(ms, 3), "triples_per_s": round(B / ms * 1e3),
           "P": P, "P_entity": P_e, "P_relation": P_r, "lstm_tflop_per_step": round(lstm_flop / 1e12, 4),
           "lstm_us_per_step": round(lstm_us, 1), "lstm_frac_of_fp32_mfma_peak": round(lstm_flop / (lstm_us * 1e-6) / 1e12 / PEAK_TFLOPS, 3),
           "kernels_us": {k: round(v, 1) for k, v in per.items()},
           "eval_precompute_entities_per_s": round(n_eval / pre_ms * 1e3)}
    del st, ps, out, raw
    torch.cuda.empty_cache()
    try:
        ref = torch_reference_step(ent_tok, rel_tok, vt_e, vt_r, d, dev)
        cand_t = [t(c.astype(np.int32)) for c in cand]
        j = [0]

        def ref_one():
            ref(batches[j[0] % 2], cand_t[j[0] % 2])
            j[0] += 1
        res["torch_rocm_ms_per_step"] = round(timed(ref_one, max(3, steps // 4), 2), 3)
        res["speedup_vs_torch_rocm"] = round(res["torch_rocm_ms_per_step"] / ms, 2)
    except torch.cuda.OutOfMemoryError as e:
        res["torch_rocm_ms_per_step"] = None
        res["torch_rocm_error"] = str(e).splitlines()[0]
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="S-FB-lstm,S-OLP-lstm")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "LSTM-encoded ComplEx training step", "results": [measure(s, dev, a.steps, a.warmup) for s in a.shapes.split(",")]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
