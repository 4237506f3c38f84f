#!/usr/bin/env python3
"""The wide path (slot sizes 513 .. 4096; csrc/okge_wide.hip): one JSON line with the dense HIP training step
(train_step.FusedTrainStep) of ComplEx at d = 1024 and d = 2048 at the S-FB shape, beside the reference's op sequence in
torch-ROCm on the same GPU in the same process (Embedding, four mm, BCEWithLogits, autograd, torch.optim.Adagrad), and the
existing d = 512 step for scale.

  S-FB   |E| = 14 543, |R| = 239, B = 512 (256 po + 256 sp), 1-vs-all (N = 14 541), input_dropout 0.4, bce

Per slot size: ms/step of both (median of nine timed windows after warm-up, min and max beside it); the HIP-event time of every
kernel of the step (okge_timing_*: per-launch mean over timed steps); each product's executed FLOP / time / 157.3 TFLOP/s -- the
score product (2 B N d) inside the train tile launch, dC = G^T . Q and dQ = G . Cm (2 B N d each) in their GEMM launches.
Usage: python tools/bench_wide.py [--steps K] [--warmup W] [--dims 512,1024,2048]
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

from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep  # noqa: E402
from bench_configs import positives_batch  # noqa: E402

PEAK_TFLOPS = 157.3                  # fp32 MFMA, MI355X
WINDOWS = 9
N_ENT, N_REL, B, P_IN = 14_543, 239, 512, 0.4


def torch_reference_step(E0, R0, dev, p_in):
    """the reference's ComplEx op sequence (model.py:198-229, :455-510; trainer.py:75-106, :221-244) in torch on the GPU"""
    n_ent, d = E0.shape
    h = d // 2
    emb_e = torch.nn.Embedding(n_ent, d, padding_idx=0).to(dev)
    emb_r = torch.nn.Embedding(R0.shape[0], d, padding_idx=0).to(dev)
    with torch.no_grad():
        emb_e.weight.copy_(E0)
        emb_r.weight.copy_(R0)
    opt = torch.optim.Adagrad([emb_e.weight, emb_r.weight], lr=0.1, weight_decay=1e-10)
    F = torch.nn.functional
    lossf = torch.nn.BCEWithLogitsLoss(reduction="sum")

    def four_mm(a, r, C, sp):
        a1, a2, r1, r2, c1, c2 = a[:, :h], a[:, h:], r[:, :h], r[:, h:], C[:, :h], C[:, h:]
        if sp:
            return (a1 * r1).mm(c1.t()) + (a2 * r1).mm(c2.t()) + (a1 * r2).mm(c2.t()) - (a2 * r2).mm(c1.t())
        return (a1 * r1).mm(c1.t()) + (a2 * r1).mm(c2.t()) + (a2 * r2).mm(c1.t()) - (a1 * r2).mm(c2.t())

    def step(batch):
        opt.zero_grad()
        C = F.dropout(emb_e.weight[2:], p_in, True)
        x_po = four_mm(F.dropout(emb_e(batch.po_obj.long()), p_in, True), emb_r(batch.po_rel.long()), C, False)
        x_sp = four_mm(F.dropout(emb_e(batch.sp_subj.long()), p_in, True), emb_r(batch.sp_rel.long()), C, True)
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


def measure(d, dev, steps, warmup):
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    E = (rng.standard_normal((N_ENT, d)) * 0.1).astype(np.float32)
    R = (rng.standard_normal((N_REL, d)) * 0.1).astype(np.float32)
    N = N_ENT - 2
    batches = [positives_batch(rng, t, N_ENT, N_REL, B, N, 2) for _ in range(4)]
    st = FusedTrainStep(t(E), t(R), "complex", lr=0.1, input_dropout=P_IN, seed=1)
    i = [0]

    def one():
        st.step(batches[i[0] % 4])
        i[0] += 1
    w_hip = windows(one, steps, warmup)
    st.engine.timing(True)                                   # per-kernel HIP-event times: a run of their own
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    kernels = {k: round(ms / max(cnt, 1) * (cnt / steps), 4) for k, (ms, cnt) in st.engine.timing_collect().items()}    # ms per step
    st.engine.timing(False)
    flop = 2.0 * B * N * d
    frac = lambda ms: round(flop / (ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3) if ms else None      # noqa: E731
    tile = kernels.get("wide_tile_train", kernels.get("fused_tile_train"))
    ref = torch_reference_step(t(E), t(R), dev, P_IN)
    j = [0]

    def ref_one():
        ref(batches[j[0] % 4])
        j[0] += 1
    w_ref = windows(ref_one, max(2, steps // 4), max(1, warmup // 2))
    ms, ms_ref = float(np.median(w_hip)), float(np.median(w_ref))
    return {"d": d, "B": B, "N": N, "path": "wide" if d > 512 else "tile kernels", "steps_per_window": steps, "windows": WINDOWS,
            "ms_per_step": round(ms, 4), "ms_per_step_min": round(min(w_hip), 4), "ms_per_step_max": round(max(w_hip), 4),
            "kernel_ms_per_step": kernels,
            "score_product_frac_of_fp32_mfma_peak": frac(tile),
            "dc_product_frac_of_fp32_mfma_peak": frac(kernels.get("wide_dc_gemm")),
            "dq_product_frac_of_fp32_mfma_peak": frac(kernels.get("wide_dq_gemm")),
            "step_frac_of_fp32_mfma_peak": round(3 * flop / (ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
            "torch_rocm_ms_per_step": round(ms_ref, 4), "torch_rocm_ms_per_step_min": round(min(w_ref), 4),
            "torch_rocm_ms_per_step_max": round(max(w_ref), 4), "speedup_vs_torch_rocm": round(ms_ref / ms, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dims", default="512,1024,2048")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "ComplEx dense training step at the S-FB shape, slot sizes 512 / 1024 / 2048",
           "results": [measure(int(d), dev, a.steps, a.warmup) for d in a.dims.split(",")]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
