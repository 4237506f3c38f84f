#!/usr/bin/env python3
"""The l2_reg hook (N3 regulariser; csrc/okge_n3.hip) beside the fused step: one JSON line, ComplEx at the S-FB shape with
d = 200 (tile kernels) and d = 2048 (the wide path).

  S-FB   |E| = 14 543, |R| = 239, B = 512 (256 po + 256 sp), 1-vs-all (N = 14 541), input_dropout 0.4, bce, l2_reg 0.01

Per slot size, ms/step (median of nine timed windows after warm-up, min and max beside it) of
  fused_step           FusedTrainStep(l2_reg=0.01)                       forward + loss + backward + the term + dense Adagrad
  fused_step_no_reg    the same step at l2_reg = 0                       what the term costs
  dropin_fused         AddLossModule(fused_l2_reg=True)  + OkgeAdagrad   the reference Trainer's calls, fused route
  dropin_fall_through  AddLossModule() on the same model + OkgeAdagrad   the only route before: torch encodes every block
  torch_adagrad        the fall-through route with torch.optim.Adagrad
and the HIP-event time of the n3 launches with the fraction of the HBM rate their 3 N d 4 bytes (candidate rows read, their
gradient rows read and written) reach.
Usage: python tools/bench_n3.py [--steps K] [--warmup W] [--dims 200,2048]
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

from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta  # noqa: E402
from open_knowledge_graph_embeddings_amd.model import Models  # noqa: E402
from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad  # noqa: E402
from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep  # noqa: E402
from open_knowledge_graph_embeddings_amd.trainer import AddLossModule  # noqa: E402
from bench_configs import positives_batch  # noqa: E402

HBM_PEAK_TBS = 8.0                   # HBM3E, MI355X (spec)
WINDOWS = 9
N_ENT, N_REL, B, P_IN, L2 = 14_543, 239, 512, 0.4, 0.01


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


def stats(w):
    return {"ms_per_step": round(float(np.median(w)), 4), "min": round(min(w), 4), "max": round(max(w), 4)}


def dropin(E, R, dev, batches, fused, optimizer):
    """the reference Trainer's calls (trainer.py:206-244): AddLossModule forward, (loss + hook) / normalizer backward, step"""
    m = Models.LookupComplexRelationModel(entity_slot_size=E.shape[1], input_dropout=P_IN, sparse=False, l2_reg=L2,
                                          train_data=EntityRelationDatasetMeta(entities_size=N_ENT, relations_size=N_REL))
    m.load_state_dict({"entity_embedding.weight": torch.from_numpy(E), "relation_embedding.weight": torch.from_numpy(R)})
    m = m.to(dev).train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False, fused_l2_reg=fused)
    opt = optimizer(m.parameters(), lr=0.1, weight_decay=1e-10)
    i = [0]

    def one():
        b = batches[i[0] % len(batches)]
        i[0] += 1
        opt.zero_grad()
        loss, hook, _ = mod(inputs=[(b.po_rel, b.po_obj), (b.sp_subj, b.sp_rel)], labels=(b.pos_row, b.pos_col),
                            use_batch_shared_entities=False, batch_shared_entities=None, epoch=1,
                            input_style_triple_or_prefix="right_and_left_prefix")
        ((loss.sum() + hook) / float(B * (N_ENT - 2))).backward()
        opt.step()
    return one


def measure(d, dev, steps, warmup):
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    E = (rng.standard_normal((N_ENT, d)) * 0.1).astype(np.float32)
    R = (rng.standard_normal((N_REL, d)) * 0.1).astype(np.float32)
    N = N_ENT - 2
    batches = [positives_batch(rng, t, N_ENT, N_REL, B, N, 2) for _ in range(4)]
    out = {"d": d, "B": B, "N": N, "path": "wide" if d > 512 else "tile kernels", "steps_per_window": steps, "windows": WINDOWS}
    for key, l2 in (("fused_step", L2), ("fused_step_no_reg", 0.0)):
        st = FusedTrainStep(t(E), t(R), "complex", lr=0.1, input_dropout=P_IN, seed=1, l2_reg=l2, l2_reg_per_direction=True)
        i = [0]

        def one():
            st.step(batches[i[0] % 4])
            i[0] += 1
        out[key] = stats(windows(one, steps, warmup))
        if l2 > 0:
            st.engine.timing(True)                                   # per-kernel HIP-event times: a run of their own
            for _ in range(steps):
                one()
            torch.cuda.synchronize()
            kernels = {k: round(ms / steps, 4) for k, (ms, cnt) in st.engine.timing_collect().items()}    # ms per step
            st.engine.timing(False)
            out["kernel_ms_per_step"] = kernels
            n3_bytes = 3.0 * N * d * 4
            out["n3_bytes_per_call"] = int(n3_bytes)
            if kernels.get("n3"):
                out["n3_frac_of_hbm_peak"] = round(n3_bytes / (kernels["n3"] * 1e-3) / 1e12 / HBM_PEAK_TBS, 3)
        del st
    slow = max(2, steps // 4)
    out["dropin_fused"] = stats(windows(dropin(E, R, dev, batches, True, OkgeAdagrad), steps, warmup))
    out["dropin_fall_through"] = stats(windows(dropin(E, R, dev, batches, False, OkgeAdagrad), slow, max(1, warmup // 2)))
    out["torch_adagrad"] = stats(windows(dropin(E, R, dev, batches, False, torch.optim.Adagrad), slow, max(1, warmup // 2)))
    out["term_cost_ms"] = round(out["fused_step"]["ms_per_step"] - out["fused_step_no_reg"]["ms_per_step"], 4)
    out["dropin_fused_vs_fall_through"] = round(out["dropin_fall_through"]["ms_per_step"] / out["dropin_fused"]["ms_per_step"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dims", default="200,2048")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"metric": "ComplEx training step with the l2_reg hook at the S-FB shape, slot sizes 200 / 2048",
           "results": [measure(int(d), dev, a.steps, a.warmup) for d in a.dims.split(",")]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
