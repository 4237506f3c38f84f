#!/usr/bin/env python3
"""Tucker3 lookup model: one JSON line with the HIP training step (tucker3.Tucker3TrainStep) at two shapes, beside the
reference's op sequence in torch-ROCm on the same GPU in the same process (Embedding, Linear, bmm, mm, BCEWithLogits, autograd,
torch.optim.Adagrad).

  S-FB-t3      |E| = 14 543, |R| = 239, d = r_e = 200, B = 512 (256 po + 256 sp), 1-vs-all, input_dropout 0.2, bce
  S-FB-t3-r30  the same with r_e = 30

Per shape: ms/step and triples/s of both (median of nine timed windows after warm-up, min and max beside it); the HIP-event time
of okge_tucker3_fold and okge_tucker3_backward alone and executed FLOP / time / 157.3 TFLOP/s (fold: 2 B d^2 r_e; backward:
d_ent + d_rel + dW = 6 B d^2 r_e); the rule `hip_below_twin_by_more_than_spread`: the HIP step's median is below the twin's
median by more than the twin's own window spread (max - min).
Usage: python tools/bench_tucker3.py [--steps K] [--warmup W] [--shapes S-FB-t3,S-FB-t3-r30]
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

from open_knowledge_graph_embeddings_amd.tucker3 import Tucker3TrainStep  # noqa: E402
from bench_configs import positives_batch  # noqa: E402

PEAK_TFLOPS = 157.3                  # fp32 MFMA, MI355X
WINDOWS = 9
SHAPES = {
    # n_ent, n_rel, d, r_e, B, input_dropout
    "S-FB-t3": (14_543, 239, 200, 200, 512, 0.2),
    "S-FB-t3-r30": (14_543, 239, 200, 30, 512, 0.2),
}


def torch_reference_step(E0, R0, W0, dev, p_in):
    """the reference's op sequence (model.py:455-510, :147-173; trainer.py:75-106, :221-244) in torch on the GPU"""
    n_ent, d = E0.shape
    emb_e = torch.nn.Embedding(n_ent, d, padding_idx=0).to(dev)
    emb_r = torch.nn.Embedding(R0.shape[0], R0.shape[1], padding_idx=0).to(dev)
    proj = torch.nn.Linear(R0.shape[1], d * d, bias=False).to(dev)
    with torch.no_grad():
        emb_e.weight.copy_(E0)
        emb_r.weight.copy_(R0)
        proj.weight.copy_(W0)
    opt = torch.optim.Adagrad([emb_e.weight, emb_r.weight, proj.weight], lr=0.1, weight_decay=1e-10)
    F = torch.nn.functional
    lossf = torch.nn.BCEWithLogitsLoss(reduction="sum")

    def step(batch):
        opt.zero_grad()
        C = F.dropout(emb_e.weight[2:], p_in, True)
        M_po = proj(emb_r(batch.po_rel.long())).view(-1, d, d)
        o = F.dropout(emb_e(batch.po_obj.long()), p_in, True)
        x_po = M_po.bmm(o.view(-1, d, 1)).view(-1, d).mm(C.t())
        s = F.dropout(emb_e(batch.sp_subj.long()), p_in, True)
        M_sp = proj(emb_r(batch.sp_rel.long())).view(-1, d, d)
        x_sp = s.view(-1, 1, d).bmm(M_sp).view(-1, d).mm(C.t())
        scores = torch.cat([x_po, x_sp])
        y = torch.zeros_like(scores)                       # (the reference's collate builds the dense labels on the host)
        y[batch.pos_row.long(), batch.pos_col.long()] = 1.0
        loss = lossf(scores.view(-1), y.view(-1))
        (loss / scores.numel()).backward()
        opt.step()
    return step


def windows(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0) / steps)
    return out


def event_ms(fn, reps=20):
    """HIP-event time of one call (median over reps, after two warm-up calls)"""
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def measure(name, dev, steps, warmup):
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    n_ent, n_rel, d, r, B, p_in = SHAPES[name]
    E = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32)
    R = (rng.standard_normal((n_rel, r)) * 0.1).astype(np.float32)
    W = (rng.standard_normal((d * d, r)) * np.sqrt(2.0 / (d * d + r))).astype(np.float32)
    N = n_ent - 2
    batches = [positives_batch(rng, t, n_ent, n_rel, B, N, 2) for _ in range(4)]
    st = Tucker3TrainStep(t(E), t(R), t(W), lr=0.1, dropout=p_in, seed=1)
    i = [0]

    def one():
        st.step(batches[i[0] % 4])
        i[0] += 1
    w_hip = windows(one, steps, warmup)
    b0 = batches[0]
    n_po, n_sp = b0.n_po, b0.n_sp
    k = st.kernels
    fold_ms = event_ms(lambda: k.fold(st.W, st.ent_rows, st.rel_rows, n_po, n_sp, st.Q))
    bwd_ms = event_ms(lambda: k.backward(st.W, st.ent_rows, st.rel_rows, st.dQ, n_po, n_sp, st.d_ent, st.d_rel, st.dW, fresh=True))
    st.dW.zero_()
    fold_flop, bwd_flop = 2.0 * B * d * d * r, 6.0 * B * d * d * r
    ref = torch_reference_step(t(E), t(R), t(W), dev, p_in)
    j = [0]

    def ref_one():
        ref(batches[j[0] % 4])
        j[0] += 1
    w_ref = windows(ref_one, steps, warmup)
    ms, ms_ref = float(np.median(w_hip)), float(np.median(w_ref))
    spread = max(w_ref) - min(w_ref)
    return {"shape": name, "d": d, "r_e": r, "B": B, "N": N, "steps_per_window": steps, "windows": WINDOWS,
            "ms_per_step": round(ms, 4), "ms_per_step_min": round(min(w_hip), 4), "ms_per_step_max": round(max(w_hip), 4),
            "triples_per_s": round(B / ms * 1e3),
            "fold_ms": round(fold_ms, 4), "fold_frac_of_fp32_mfma_peak": round(fold_flop / (fold_ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
            "backward_ms": round(bwd_ms, 4), "backward_frac_of_fp32_mfma_peak": round(bwd_flop / (bwd_ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
            "torch_rocm_ms_per_step": round(ms_ref, 4), "torch_rocm_ms_per_step_min": round(min(w_ref), 4),
            "torch_rocm_ms_per_step_max": round(max(w_ref), 4), "torch_rocm_triples_per_s": round(B / ms_ref * 1e3),
            "speedup_vs_torch_rocm": round(ms_ref / ms, 2),
            "hip_below_twin_by_more_than_spread": bool(ms_ref - ms > spread)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="S-FB-t3,S-FB-t3-r30")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "Tucker3 lookup model training step", "results": [measure(s, dev, a.steps, a.warmup) for s in a.shapes.split(",")]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
