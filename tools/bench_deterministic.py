#!/usr/bin/env python3
"""What the deterministic dense step costs: FusedTrainStep(deterministic=True) beside the default step and the row-sparse step
with deferred weight decay, all at the reference's weight_decay = 1e-10.

  S-FB   ComplEx d = 200, B = 512 (256 po + 256 sp), 1-vs-all over |E| = 14 543 (candidates 2 .. 14 542), |R| = 239, dropout 0.4
  S-DM   DistMult d = 512, B = 512, 10 000 sampled candidates of |E| = 14 543, |R| = 240

default        = FusedTrainStep(): prefix contributions added with float atomics in arrival order
deterministic  = FusedTrainStep(deterministic=True): occurrence rows + okge_rows_to_dense, then the same dense tail
sparse W=16    = FusedTrainStep(sparse=True, decay_window=16): okge_rows_catch_up + okge_adagrad_rows_decay

Method (tools/bench_sparse.py): every step is warmed up, then timed in windows of >= 0.25 s of back-to-back eager steps over four
rotating batches, ending in a device synchronise; the three steps ALTERNATE window by window and the median window is reported
with the range (min, max) beside it.  The per-kernel split comes from a run of its own with the library's HIP-event timers on.
Needs an MI355X.  Prints markdown and one JSON line; --out writes the markdown to a file.

    python tools/bench_deterministic.py --out profiles/deterministic_measured.md
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_sparse import kernel_split, make_batches, measure      # noqa: E402

WD = 1e-10
SHAPES = [  # name, scorer, d, B, N (0: 1-vs-all from row 2), n_ent, n_rel, input dropout
    ("S-FB", "complex", 200, 512, 0, 14_543, 239, 0.4),
    ("S-DM", "distmult", 512, 512, 10_000, 14_543, 240, 0.2),
]
LABELS = ["default", "deterministic", "sparse W=16"]


def range_batches(dev, n_ent, n_rel, B, count=4):
    """1-vs-all: the candidate range 2 .. n_ent - 1, two positives per row"""
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch
    out, N = [], n_ent - 2
    for _ in range(count):
        ri = lambda hi, n: torch.randint(2, hi, (n,), device=dev, dtype=torch.int32)      # noqa: E731
        col = torch.randint(0, N, (2 * B,), device=dev, dtype=torch.int32)
        row = torch.arange(B, device=dev, dtype=torch.int32).repeat(2)
        order = torch.argsort(col, stable=True)
        out.append(PrefixBatch(po_rel=ri(n_rel, B // 2), po_obj=ri(n_ent, B // 2), sp_subj=ri(n_ent, B - B // 2), sp_rel=ri(n_rel, B - B // 2),
                               pos_row=row[order].contiguous(), pos_col=col[order].contiguous(), cand_first=2, n_cand=N))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="comma-separated subset of S-FB,S-DM")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deterministic.py measures on an MI355X; there is no CPU path")
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    only = set(args.only.split(",")) if args.only else None
    dev = torch.device("cuda:0")
    hp = HotPath(dev)
    lines, splits, result = [], [], {}
    for name, scorer, d, B, N, n_ent, n_rel, p in SHAPES:
        if only and name not in only:
            continue
        torch.manual_seed(d + n_ent)
        batches = make_batches(dev, n_ent, n_rel, B, N) if N else range_batches(dev, n_ent, n_rel, B)
        kws = {"default": {}, "deterministic": dict(deterministic=True), "sparse W=16": dict(sparse=True, decay_window=16)}
        steps = {}
        for label in LABELS:
            E = torch.randn((n_ent, d), device=dev) * 0.1
            R = torch.randn((n_rel, d), device=dev) * 0.1
            steps[label] = FusedTrainStep(E, R, scorer, lr=0.3, weight_decay=WD, eps=1e-8, input_dropout=p, seed=1, engine=hp, **kws[label])
        counters = {k: 0 for k in LABELS}

        def make(label):
            def fn():
                counters[label] += 1
                steps[label].step(batches[counters[label] % len(batches)])
            return fn
        fns = {k: make(k) for k in LABELS}
        cands = f"N = {N} sampled" if N else f"1-vs-all (N = {n_ent - 2})"
        lines += [f"### {name}: {scorer} d = {d}, B = {B}, {cands}, |E| = {n_ent}, |R| = {n_rel}", "",
                  "| step | ms per step, median (min, max) | against default |", "|---|---|---|"]
        t, iters = measure(fns, args.windows, args.warmup)
        result[name] = {}
        for label in LABELS:
            m, lo, hi = t[label]
            lines.append(f"| {label} | {m:.3f} ({lo:.3f}, {hi:.3f}) | {m / t['default'][0]:.2f}x |")
            result[name][label] = {"ms": round(m, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4)}
            splits.append(f"- {name} {label}: " + kernel_split(hp, fns[label], max(3, iters[label] // 4)))
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
    print(json.dumps({"bench": "deterministic_step", **result}))


if __name__ == "__main__":
    main()
