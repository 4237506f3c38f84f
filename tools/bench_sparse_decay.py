#!/usr/bin/env python3
"""Row-sparse training step with deferred weight decay against the dense step at the reference's weight_decay = 1e-10.

  (a) ComplEx d = 256, B = 4096, N = 8192 sampled candidates, |E| = 250 000, |R| = 100 000
  (b) the same at |E| = 2 500 000
  (c) S-DM: DistMult d = 512, B = 512, N = 10 000, |E| = 14 543

dense     = FusedTrainStep(weight_decay=1e-10): dense dE / dR, adagrad2 over both tables (the parent commit's only way to train
            with the reference's weight decay)
sparse wd0 = FusedTrainStep(weight_decay=0, sparse=True): okge_adagrad_rows, no decay at all (the floor)
W = k     = FusedTrainStep(weight_decay=1e-10, sparse=True, decay_window=k): okge_rows_catch_up + okge_adagrad_rows_decay

Method (tools/bench_sparse.py): every configuration is warmed up, then timed in windows of >= 0.25 s of back-to-back steps over
four rotating batches, ending in a device synchronise; the configurations alternate window by window and the MEDIAN window is
reported (min / max beside it).  Each shape is measured twice: from fresh (cold) accumulators, and again after --warm-steps
further steps of every configuration.  flush() is timed with HIP events right after W steps (the lag a reader would meet), the
median of three.  The per-kernel split comes from a run of its own with the library's HIP-event timers on.
Needs an MI355X.  Prints markdown and one JSON line; --out writes the markdown to a file.

    python tools/bench_sparse_decay.py --out profiles/sparse_decay_measured.md
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparse import SHAPES, kernel_split, make_batches, measure      # noqa: E402

WINDOWS = (1, 2, 4, 8, 16, 32)
WD = 1e-10


def flush_ms(step, fn, w):
    out = []
    for _ in range(3):
        for _ in range(max(w, 1)):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step.flush()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--warm-steps", type=int, default=200)
    ap.add_argument("--only", default=None, help="comma-separated subset of a,b,c")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_decay.py measures on an MI355X; there is no CPU path")
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    only = set(args.only.split(",")) if args.only else None
    dev = torch.device("cuda:0")
    hp = HotPath(dev)
    labels = ["dense", "sparse wd0"] + [f"W={w}" for w in WINDOWS]
    lines, splits, result = [], [], {}
    for name, scorer, d, B, N, n_ent, n_rel in SHAPES:
        if only and name not in only:
            continue
        torch.manual_seed(d + n_ent)
        batches = make_batches(dev, n_ent, n_rel, B, N)
        steps = {}
        for label in labels:
            E = torch.randn((n_ent, d), device=dev) * 0.1
            R = torch.randn((n_rel, d), device=dev) * 0.1
            kw = {} if label == "dense" else dict(sparse=True)
            if label.startswith("W="):
                kw["decay_window"] = int(label[2:])
            steps[label] = FusedTrainStep(E, R, scorer, lr=0.3, weight_decay=0.0 if label == "sparse wd0" else WD, eps=1e-8,
                                          input_dropout=0.2, seed=1, engine=hp, **kw)
        counters = {k: 0 for k in labels}

        def make(label):
            def fn():
                counters[label] += 1
                steps[label].step(batches[counters[label] % len(batches)])
            return fn
        fns = {k: make(k) for k in labels}
        lines += [f"### ({name}) {scorer} d = {d}, B = {B}, N = {N}, |E| = {n_ent}", "",
                  "| step | cold ms (min, max) | after " + str(args.warm_steps) + " steps ms (min, max) | flush ms cold | flush ms warm |",
                  "|---|---|---|---|---|"]
        cold, iters = measure(fns, args.windows, args.warmup)
        fl_cold = {k: flush_ms(steps[k], fns[k], int(k[2:])) for k in labels if k.startswith("W=")}
        for label in labels:
            splits.append(f"- ({name}) cold {label}: " + kernel_split(hp, fns[label], max(3, iters[label] // 4)))
        for fn in fns.values():
            for _ in range(args.warm_steps):
                fn()
        warm, _ = measure(fns, args.windows, 0)
        fl_warm = {k: flush_ms(steps[k], fns[k], int(k[2:])) for k in labels if k.startswith("W=")}
        for label in labels:
            splits.append(f"- ({name}) warm {label}: " + kernel_split(hp, fns[label], max(3, iters[label] // 4)))
        result[name] = {}
        for label in labels:
            (mc, lc, hc), (mw, lw, hw) = cold[label], warm[label]
            fc = f"{fl_cold[label]:.3f}" if label in fl_cold else "-"
            fw = f"{fl_warm[label]:.3f}" if label in fl_warm else "-"
            lines.append(f"| {label} | {mc:.3f} ({lc:.3f}, {hc:.3f}) | {mw:.3f} ({lw:.3f}, {hw:.3f}) | {fc} | {fw} |")
            result[name][label] = {"cold_ms": round(mc, 4), "warm_ms": round(mw, 4)}
        lines.append("")
        del steps, fns, batches
        torch.cuda.empty_cache()
    text = ("\n".join(lines) + "\nPer-kernel split (HIP events around every library launch, ms per step x launches per step):\n\n"
            + "\n".join(splits) + "\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "sparse_decay_step", **result}))


if __name__ == "__main__":
    main()
