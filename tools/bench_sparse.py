#!/usr/bin/env python3
"""Row-sparse training step against the dense one, both at weight_decay = 0, on batch-shared sampled candidates.

  (a) ComplEx d = 256, B = 4096, N = 8192 sampled candidates, |E| = 250 000, |R| = 100 000
  (b) the same at |E| = 2 500 000 (S-OLP, batch-shared variant of SURVEY section 8d)
  (c) S-DM: DistMult d = 512, B = 512, N = 10 000, |E| = 14 543
  (d) the drop-in path -- AddLossModule + OkgeAdagrad -- at (a), dense gradients against sparse_grads=True

dense  = FusedTrainStep(weight_decay=0): dense dE / dR, cleared when a sampled list leaves rows untouched, adagrad2 over both tables
sparse = FusedTrainStep(weight_decay=0, sparse=True): occurrence rows + okge_adagrad_rows

Method (tools/bench_topk.py): every configuration is warmed up, then timed in windows of >= 0.25 s of back-to-back steps over
four rotating batches, ending in a device synchronise; dense and sparse alternate window by window and the MEDIAN window is
reported (min / max beside it).  The per-kernel split comes from a run of its own with the library's HIP-event timers on.
Needs an MI355X.  Prints a markdown table and one JSON line; --out writes the markdown to a file.

    python tools/bench_sparse.py --out profiles/sparse_measured.md
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # name, scorer, d, B, N, n_ent, n_rel
    ("a", "complex", 256, 4096, 8192, 250_000, 100_000),
    ("b", "complex", 256, 4096, 8192, 2_500_000, 100_000),
    ("c", "distmult", 512, 512, 10_000, 14_543, 240),
]


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def make_batches(dev, n_ent, n_rel, B, N, count=4):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch
    out = []
    for _ in range(count):
        ri = lambda hi, n: torch.randint(2, hi, (n,), device=dev, dtype=torch.int32)      # noqa: E731
        cand = (torch.randperm(n_ent - 2, device=dev)[:N] + 2).to(torch.int32)
        col = torch.randint(0, N, (2 * B,), device=dev, dtype=torch.int32)
        row = torch.arange(B, device=dev, dtype=torch.int32).repeat(2)
        order = torch.argsort(col, stable=True)
        out.append(PrefixBatch(po_rel=ri(n_rel, B // 2), po_obj=ri(n_ent, B // 2), sp_subj=ri(n_ent, B - B // 2), sp_rel=ri(n_rel, B - B // 2),
                               pos_row=row[order].contiguous(), pos_col=col[order].contiguous(), cand_ids=cand, cand_unique=True))
    return out


def measure(fns, windows, warmup):
    """fns: {label: step function}; alternating windows -> {label: (median, min, max) ms}, iterations per window"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    iters = {k: max(3, math.ceil(0.25 / window(fn, 3))) for k, fn in fns.items()}
    t = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            t[k].append(window(fn, iters[k]) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}, iters


def kernel_split(hp, fn, n_calls):
    hp.timing(True)
    for _ in range(n_calls):
        fn()
    torch.cuda.synchronize()
    t = hp.timing_collect()
    hp.timing(False)
    return ", ".join(f"`{kn}` {ms / n_calls:.4f} ms x {cnt / n_calls:g}" for kn, (ms, cnt) in sorted(t.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated subset of a,b,c,d")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse.py measures on an MI355X; there is no CPU path")
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    only = set(args.only.split(",")) if args.only else None
    dev = torch.device("cuda:0")
    hp = HotPath(dev)
    lines = ["| shape | path | scorer | d | B | N | |E| | dense ms | sparse ms | dense / sparse |", "|---|---|---|---|---|---|---|---|---|---|"]
    splits, result = [], {}

    def report(name, path, scorer, d, B, N, n_ent, t):
        (md, lo_d, hi_d), (ms, lo_s, hi_s) = t["dense"], t["sparse"]
        lines.append(f"| {name} | {path} | {scorer} | {d} | {B} | {N} | {n_ent} | {md:.3f} (min {lo_d:.3f}, max {hi_d:.3f}) | "
                     f"{ms:.3f} (min {lo_s:.3f}, max {hi_s:.3f}) | {md / ms:.2f} |")
        result[name] = {"dense_ms": round(md, 4), "sparse_ms": round(ms, 4)}

    for name, scorer, d, B, N, n_ent, n_rel in SHAPES:
        if only and name not in only:
            continue
        torch.manual_seed(d + n_ent)
        batches = make_batches(dev, n_ent, n_rel, B, N)
        steps = {}
        for label in ("dense", "sparse"):
            E = torch.randn((n_ent, d), device=dev) * 0.1
            R = torch.randn((n_rel, d), device=dev) * 0.1
            steps[label] = FusedTrainStep(E, R, scorer, lr=0.3, weight_decay=0.0, eps=1e-8, input_dropout=0.2, seed=1, engine=hp,
                                          sparse=(label == "sparse"))
        counters = {"dense": 0, "sparse": 0}

        def make(label):
            def fn():
                counters[label] += 1
                steps[label].step(batches[counters[label] % len(batches)])
            return fn
        fns = {k: make(k) for k in steps}
        t, iters = measure(fns, args.windows, args.warmup)
        report(name, "FusedTrainStep", scorer, d, B, N, n_ent, t)
        for label in ("dense", "sparse"):
            splits.append(f"- ({name}) {label}: " + kernel_split(hp, fns[label], max(3, iters[label] // 4)))
        del steps, fns, batches
        torch.cuda.empty_cache()

    if not only or "d" in only:
        from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
        from open_knowledge_graph_embeddings_amd.model import Models
        from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
        from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
        _, scorer, d, B, N, n_ent, n_rel = SHAPES[0]
        torch.manual_seed(7)
        batches = make_batches(dev, n_ent, n_rel, B, N)
        fns = {}
        for label in ("dense", "sparse"):
            m = Models.LookupComplexRelationModel(entity_slot_size=d, input_dropout=0.2, init_std=0.1, sparse=False,
                                                  train_data=EntityRelationDatasetMeta(entities_size=n_ent, relations_size=n_rel)).to(dev).train()
            mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False,
                                sparse_grads=(label == "sparse")).train()
            opt = OkgeAdagrad(m.parameters(), lr=0.3, weight_decay=0, eps=1e-8)
            state = {"i": 0}

            def fn(mod=mod, opt=opt, state=state):
                state["i"] += 1
                b = batches[state["i"] % len(batches)]
                opt.zero_grad()
                loss, _, _ = mod(inputs=[(b.po_rel, b.po_obj), (b.sp_subj, b.sp_rel)], labels=(b.pos_row, b.pos_col),
                                 use_batch_shared_entities=True, batch_shared_entities=b.cand_ids, epoch=1,
                                 input_style_triple_or_prefix="right_and_left_prefix")
                (loss.sum() / float(B * N)).backward()
                opt.step()
            fns[label] = fn
        t, iters = measure(fns, args.windows, args.warmup)
        report("d", "AddLossModule + OkgeAdagrad", scorer, d, B, N, n_ent, t)
        for label in ("dense", "sparse"):
            splits.append(f"- (d) {label}: " + kernel_split(hp, fns[label], max(3, iters[label] // 4))
                          + "  (+ torch's own allocation / fill kernels, not library launches)")

    if "a" in result and "b" in result:
        result["b_over_a"] = {"dense": round(result["b"]["dense_ms"] / result["a"]["dense_ms"], 3),
                              "sparse": round(result["b"]["sparse_ms"] / result["a"]["sparse_ms"], 3)}
    text = ("\n".join(lines) + "\n\nPer-kernel split (HIP events around every library launch, ms per step x launches per step):\n\n"
            + "\n".join(splits) + "\n")
    if "b_over_a" in result:
        text += (f"\n(b) / (a), the tables ten times as large: dense {result['b_over_a']['dense']:.2f}, "
                 f"sparse {result['b_over_a']['sparse']:.2f}\n")
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"bench": "sparse_step", **result}))


if __name__ == "__main__":
    main()
