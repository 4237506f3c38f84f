#!/usr/bin/env python3
"""Lookup embedder variants: one JSON line with the HIP training step (lookup_variants.LookupVariantTrainStep, Adagrad) beside the
unchanged torch fall-through (trainer.AddLossModule + optim.OkgeAdagrad: torch encodes, HIP scores) on the same GPU, at the S-FB
shape: ComplEx d = 200, |E| = 14 543, B = 512, 1-vs-all (N = 14 541), BCE.

  bn    batch_norm=True, input_dropout=0.2
  all   batch_norm, project_entity (ReLU), normalize='norm', l2_reg=0.01, input_dropout=0.2

The two sides run in alternating windows of --steps steps (host clock around a device synchronise), --rounds times; the medians
and every window are reported.  Then, in a separate pass with HIP-event timing on, the time per step of each entry point of
the HIP step.  --hip-only runs nothing but the HIP step's windows: the run to put under `rocprofv3 --kernel-trace --stats`
for the per-kernel table.
Usage: python tools/bench_lookup_variants.py [--steps K] [--warmup W] [--rounds R] [--configs bn,all] [--hip-only]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta  # noqa: E402
from open_knowledge_graph_embeddings_amd.model import Models  # noqa: E402
from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad  # noqa: E402
from open_knowledge_graph_embeddings_amd.trainer import AddLossModule  # noqa: E402
from bench_configs import positives_batch  # noqa: E402

N_ENT, N_REL, D, B = 14_543, 239, 200, 512
CONFIGS = {
    "bn": dict(batch_norm=True, input_dropout=0.2),
    "all": dict(batch_norm=True, project_entity=True, normalize="norm", l2_reg=0.01, input_dropout=0.2),
}


def build(kw, dev):
    torch.manual_seed(1)
    m = Models.LookupComplexRelationModel(entity_slot_size=D, train_data=EntityRelationDatasetMeta(entities_size=N_ENT, relations_size=N_REL),
                                          init_std=0.1, seed=1, **kw)
    return m.cuda().train()


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def measure(name, dev, steps, warmup, rounds, hip_only=False):
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    N = N_ENT - 2
    batches = [positives_batch(rng, t, N_ENT, N_REL, B, N, 2) for _ in range(4)]
    cand = t(np.arange(2, N_ENT, dtype=np.int32))
    hip_model, torch_model = build(CONFIGS[name], dev), build(CONFIGS[name], dev)
    st = hip_model.train_step(lr=0.1)
    mod = AddLossModule(torch_model, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False)
    opt = OkgeAdagrad(torch_model.parameters(), lr=0.1, weight_decay=1e-10, eps=1e-8)
    i, j = [0], [0]

    def hip_step():
        st.step(batches[i[0] % 4])
        i[0] += 1

    def fall_through_step():
        b = batches[j[0] % 4]
        j[0] += 1
        opt.zero_grad()
        loss, hook, _ = mod(inputs=[(b.po_rel, b.po_obj), (b.sp_subj, b.sp_rel)], labels=(b.pos_row, b.pos_col), use_batch_shared_entities=False,
                            batch_shared_entities=cand, epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
        total = loss.sum() if hook is None else loss.sum() + hook
        (total / float(B * N)).backward()
        opt.step()
    if hip_only:
        for _ in range(warmup):
            hip_step()
        hip_ms = [window(hip_step, steps) for _ in range(rounds)]
        return {"config": name, "settings": CONFIGS[name], "d": D, "B": B, "N": N, "hip_step_ms": round(statistics.median(hip_ms), 3),
                "hip_windows_ms": [round(x, 3) for x in hip_ms]}
    for _ in range(warmup):
        hip_step()
        fall_through_step()
    hip_ms, torch_ms = [], []
    for _ in range(rounds):
        hip_ms.append(window(hip_step, steps))
        torch_ms.append(window(fall_through_step, steps))
    st.engine.timing(True)
    n_timed = 8
    for _ in range(n_timed):
        hip_step()
    torch.cuda.synchronize()
    per = {k: round(v[0] / n_timed * 1e3, 1) for k, v in st.engine.timing_collect().items()}
    st.engine.timing(False)
    h, f = statistics.median(hip_ms), statistics.median(torch_ms)
    return {"config": name, "settings": CONFIGS[name], "d": D, "B": B, "N": N,
            "hip_step_ms": round(h, 3), "fall_through_ms": round(f, 3), "fall_through_over_hip": round(f / h, 2),
            "hip_windows_ms": [round(x, 3) for x in hip_ms], "fall_through_windows_ms": [round(x, 3) for x in torch_ms],
            "hip_entry_points_us_per_step": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="bn,all")
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "lookup embedder variants, ComplEx d=200 S-FB training step: HIP step vs torch fall-through",
           "results": [measure(c, dev, a.steps, a.warmup, a.rounds, a.hip_only) for c in a.configs.split(",")]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
