#!/usr/bin/env python3
"""Bigram-pooling models: one JSON line with the HIP training step (bigram.BigramTrainStep) at two shapes, beside the
reference's op sequence in torch-ROCm on the same GPU (nn.Embedding, nn.Conv1d = MIOpen, nn.BatchNorm1d(momentum=None), ATen for
the rest, torch.optim.Adagrad).

  S-FB-bigram   ComplEx d=512, |E| = 14 543, B = 4096, 1-vs-all (N = 14 541), batch-norm, sum pooling, dropout 0.1, max_len 10
                (synthetic Zipf mention tokens)
  S-OLP-bigram  ComplEx d=512, 2.5 M entities with synthetic tokens (synthetic.make_token_matrix), B = 4096, batch-shared
                N = 4096, batch-norm, sum pooling, dropout 0.1

Per shape: step ms and triples/s; P = rows x (max_len - 1), the positions of the pair product (all of them enter the batch-norm
statistics); product FLOP per step (4 P d^2 forward + 8 P d^2 backward); the bigram calls' HIP-event time
(okge_bigram_encode_calls + okge_bigram_backward_calls: product, statistics, pooling, weight gradients, scatter) and the FLOP
share of the fp32-MFMA peak in it; eval precompute entities/s; the torch-ROCm step.
Usage: python tools/bench_bigram.py [--steps K] [--warmup W] [--shapes S-FB-bigram,S-OLP-bigram]
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

from open_knowledge_graph_embeddings_amd.bigram import BigramPass, BigramSlot, BigramTrainStep, PRECOMPUTE_CHUNK  # noqa: E402
from open_knowledge_graph_embeddings_amd.synthetic import make_token_matrix  # noqa: E402
from bench_configs import positives_batch  # noqa: E402

PEAK_TFLOPS = 157.3                  # fp32 MFMA, MI355X
SHAPES = {
    # n_ent, n_rel, vocab_e, vocab_r, d, B, N (None: 1-vs-all), max_len
    "S-FB-bigram": (14_543, 239, 30_000, 2_000, 512, 4096, None, 10),
    "S-OLP-bigram": (2_500_000, 100_000, 200_000, 50_000, 512, 4096, 4096, 10),
}


def make_slot(dev, vocab, tok, d):
    b = 1.0 / np.sqrt(2 * d)
    return BigramSlot(torch.randn((vocab, d), device=dev) * 0.1, torch.from_numpy(tok).to(dev),
                      torch.empty((d, d, 2), device=dev).uniform_(-b, b), "sum", "batchnorm",
                      (torch.ones(d, device=dev), torch.zeros(d, device=dev)))


def torch_reference_step(ent_tok, rel_tok, vt_e, vt_r, d, dev, dropout=0.1):
    """the reference's op sequence (model.py:874-897 behind the id -> token mapping, + :198-229 + trainer.py:75-106, 221-244)
    in torch on the GPU"""
    emb_e = torch.nn.Embedding(vt_e, d, padding_idx=0).to(dev)
    emb_r = torch.nn.Embedding(vt_r, d, padding_idx=0).to(dev)
    enc_e = torch.nn.Sequential(torch.nn.Conv1d(d, d, 2, bias=False), torch.nn.BatchNorm1d(d, momentum=None)).to(dev)
    enc_r = torch.nn.Sequential(torch.nn.Conv1d(d, d, 2, bias=False), torch.nn.BatchNorm1d(d, momentum=None)).to(dev)
    params = [emb_e.weight, emb_r.weight, *enc_e.parameters(), *enc_r.parameters()]
    opt = torch.optim.Adagrad(params, lr=0.1, weight_decay=1e-10)
    te, tr = torch.from_numpy(ent_tok).to(dev).long(), torch.from_numpy(rel_tok).to(dev).long()
    h = d // 2

    def enc(ids, tok, emb, encoder):
        x = tok[ids.long()]
        mask = (x > 0).unsqueeze(1).float()[:, :, 1:]
        embedded = emb(x).transpose(1, 2)
        encoded = encoder(embedded) + embedded[:, :, 1:]
        return torch.nn.functional.dropout((encoded * mask).sum(dim=2), dropout, True)

    def step(batch, cand):
        opt.zero_grad()
        C = enc(cand, te, emb_e, enc_e)
        r_po, o = enc(batch.po_rel, tr, emb_r, enc_r), enc(batch.po_obj, te, emb_e, enc_e)
        s, r_sp = enc(batch.sp_subj, te, emb_e, enc_e), enc(batch.sp_rel, tr, emb_r, enc_r)
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
    ent, rel = make_slot(dev, vt_e, ent_tok, d), make_slot(dev, vt_r, rel_tok, d)
    st = BigramTrainStep(ent, rel, "complex", lr=0.1, dropout=0.1, seed=1)
    if N is None:
        batches = [positives_batch(rng, t, n_ent, n_rel, B, n_ent - 2, 2) for _ in range(2)]
        cand = [np.arange(2, n_ent)] * 2
    else:
        cids = [rng.choice(n_ent - 2, N, replace=False).astype(np.int32) + 2 for _ in range(2)]
        batches = [positives_batch(rng, t, n_ent, n_rel, B, N, 1, cand_ids=t(c)) for c in cids]
        cand = cids
    rows_e, rows_r = len(cand[0]) + B, B
    P = (rows_e + rows_r) * (L - 1)
    live = int((ent_tok[np.concatenate([cand[0], batches[0].po_obj.cpu().numpy(), batches[0].sp_subj.cpu().numpy()])][:, 1:] > 0).sum())
    flop = 12.0 * P * d * d
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
    bg_us = 2 * (per.get("bigram_encode", 0.0) + per.get("bigram_backward", 0.0))       # two passes (entity, relation) per step
    # eval precompute: entity rows in PRECOMPUTE_CHUNK-row encode calls, running statistics
    n_eval = min(n_ent, 16 * PRECOMPUTE_CHUNK)
    ps, out = BigramPass(dev), torch.empty((PRECOMPUTE_CHUNK, d), device=dev)

    def pre():
        for lo in range(0, n_eval, PRECOMPUTE_CHUNK):
            m = min(PRECOMPUTE_CHUNK, n_eval - lo)
            ps.encode(ent, [(None, lo, m)], False, out[:m])
    pre_ms = timed(pre, 3, 1)
    res = {"shape": name, "d": d, "B": B, "N": N if N is not None else n_ent - 2, "max_len": L,
           "ms_per_step": round(ms, 3), "triples_per_s": round(B / ms * 1e3),
           "P": P, "live_entity_positions": live, "product_tflop_per_step": round(flop / 1e12, 4),
           "bigram_us_per_step": round(bg_us, 1),
           "bigram_frac_of_fp32_mfma_peak": round(flop / max(bg_us, 1e-9) / 1e-6 / 1e12 / PEAK_TFLOPS, 3),
           "kernels_us": {k: round(v, 1) for k, v in per.items()},
           "eval_precompute_entities_per_s": round(n_eval / pre_ms * 1e3)}
    del st, ps, out
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
    ap.add_argument("--shapes", default="S-FB-bigram,S-OLP-bigram")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "bigram-pooling ComplEx training step", "results": [measure(s, dev, a.steps, a.warmup) for s in a.shapes.split(",")]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
