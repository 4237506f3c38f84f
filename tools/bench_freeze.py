#!/usr/bin/env python3
"""FusedTrainStep(freeze=...) on one GPU at the two lookup shapes of bench_configs.py (profiles/freeze.md holds the tables):

  S-FB   ComplEx d = 200, B = 512, 1-vs-all over 14 541 entities (the bench.py workload)
  S-DM   DistMult d = 512, B = 512, a batch-shared sampled list of 10 000 unique candidates

  default   the step with default keywords -- the line to compare between two commits: it passes no `freeze` keyword, so a
            checkout from before the keyword runs it too.  Run it from both trees in turn (this, parent, this, parent) with
            --label naming the tree; the margin of the comparison is the spread of the parent's own runs
  freeze    freeze=None, "entities" and "relations": eager ms/step and the per-kernel times (okge_timing_*); run from a parent
            that has the keyword too, it is compared like the default line

Every step figure is the median of `--windows` windows of `--steps` steps, each window closed by a device synchronise, with the
fastest and slowest window beside it.  One JSON object per line; `--report OUT.md LOG [LOG ...]` turns the logs of such runs into
the markdown tables.  Whatever OUT.md holds from its "## Reading" heading on -- the hand-written reading of the numbers -- is kept;
a new file gets an empty one.

The run behind profiles/freeze.md, with PARENT a checkout of the parent commit, built, with this file copied into its tools/:

    for i in 0 1; do
        python PARENT/tools/bench_freeze.py --only default --label parent >> default.jsonl
        python tools/bench_freeze.py --only default --label this >> default.jsonl
    done
    python tools/bench_freeze.py --only freeze > modes.jsonl
    python tools/bench_freeze.py --report profiles/freeze.md default.jsonl modes.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def setup(shape, dev, **kw):
    """(step, resident batches) of `shape` under the keywords kw (the seeds of bench_configs.py: the same problem)"""
    import numpy as np
    import torch
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    import bench_configs
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    if shape == "S-DM":
        rng = np.random.default_rng(1)
        n_ent, n_rel, d, B, N = 14543, 239, 512, 512, 10000
        E, R = (rng.standard_normal((n, d), dtype=np.float32) * 0.1 for n in (n_ent, n_rel))
        step = FusedTrainStep(t(E), t(R), "distmult", lr=0.1, input_dropout=0.2, seed=1, **kw)
        batches = [bench_configs.positives_batch(rng, t, n_ent, n_rel, B, N, 2, cand_ids=t(rng.permutation(np.arange(2, n_ent))[:N].astype(np.int32)),
                                                 cand_unique=True) for _ in range(4)]
        return step, batches
    from open_knowledge_graph_embeddings_amd import synthetic
    w = synthetic.WORKLOADS["S-FB"]
    E, R = synthetic.make_tables(w, seed=1234)
    step = FusedTrainStep(t(E), t(R), w.scorer, lr=w.lr, input_dropout=w.input_dropout, seed=1, **kw)
    batches = []
    for i in range(4):
        hb = synthetic.make_batch(w, seed=1234 + i)
        batches.append(H.PrefixBatch(po_rel=t(hb["po_rel"]), po_obj=t(hb["po_obj"]), sp_subj=t(hb["sp_subj"]), sp_rel=t(hb["sp_rel"]),
                                     pos_row=t(hb["pos_row"]), pos_col=t(hb["pos_col"]), cand_first=2, n_cand=w.N))
    return step, batches


def measure(shape, dev, args, label, **kw):
    import torch
    step, batches = setup(shape, dev, **kw)
    for i in range(args.warmup):
        step.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.windows):
        t0 = time.perf_counter()
        for i in range(args.steps):
            step.step(batches[i % len(batches)])
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / args.steps)
    eng = step.engine
    eng.timing(True)
    for i in range(args.ksteps):
        step.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    per = {k: round(v[0] / v[1] * 1e3, 2) for k, v in eng.timing_collect().items()}
    eng.timing(False)
    out = {"build": label, "shape": shape, "freeze": kw.get("freeze"), "keyword_passed": "freeze" in kw,
           "ms_per_step_median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
           "windows": args.windows, "steps": args.steps, "kernels_us": per}
    print(json.dumps(out), flush=True)
    del step, batches
    torch.cuda.empty_cache()
    return out


def compare(rows):
    """per (shape, freeze) measured from both trees: the medians of each, the difference of their means, the parent's own spread
    -- the margin of the comparison -- and the runs of this tree that lie outside the parent's range"""
    text = []
    for shape, freeze in sorted({(r["shape"], str(r["freeze"])) for r in rows}):
        by = {}
        for r in rows:
            if (r["shape"], str(r["freeze"])) == (shape, freeze):
                by.setdefault(r["build"], []).append(r["ms_per_step_median"])
        if "parent" in by and "this" in by:
            lo, hi = min(by["parent"]), max(by["parent"])
            delta = statistics.mean(by["this"]) - statistics.mean(by["parent"])
            outside = [x for x in by["this"] if not lo <= x <= hi]
            text.append(f"{shape}, freeze {freeze}: parent {by['parent']}, this {by['this']}; this - parent = {delta:+.4f} ms, the parent's "
                        f"own spread {hi - lo:.4f} ms; runs of this tree outside [{lo}, {hi}]: {outside or 'none'}.")
    return text


def report(out_path, logs):
    rows = []
    for path in logs:
        with open(path) as f:
            rows += [json.loads(line) for line in f if line.startswith("{")]
    default = [r for r in rows if not r["keyword_passed"]]
    frozen = [r for r in rows if r["keyword_passed"]]
    text = ["# FusedTrainStep(freeze=...): step times (tools/bench_freeze.py)", "",
            "Eager ms/step: the median of the windows, fastest and slowest window beside it.", "",
            "## The default step, this build and the parent commit in turn", "",
            "| run | build | shape | ms/step | min | max |", "|---|---|---|---|---|---|"]
    for i, r in enumerate(default):
        text.append(f"| {i} | {r['build']} | {r['shape']} | {r['ms_per_step_median']:.4f} | {r['min']:.4f} | {r['max']:.4f} |")
    text += [""] + compare(default)
    text += ["", "## freeze=None, \"entities\", \"relations\"", "",
             "| build | shape | freeze | ms/step | min | max |", "|---|---|---|---|---|---|"]
    for r in frozen:
        text.append(f"| {r['build']} | {r['shape']} | {r['freeze']} | {r['ms_per_step_median']:.4f} | {r['min']:.4f} | {r['max']:.4f} |")
    text += [""] + compare(frozen)
    text += ["", "## Per-kernel times of those runs (okge_timing_*, us per launch)", ""]
    names = sorted({k for r in frozen for k in r["kernels_us"]})
    text += ["| build | shape | freeze | " + " | ".join(names) + " |", "|---|---|---|" + "---|" * len(names)]
    for r in frozen:
        text.append(f"| {r['build']} | {r['shape']} | {r['freeze']} | " + " | ".join(str(r["kernels_us"].get(k, "-")) for k in names) + " |")
    reading = "## Reading\n\n(not written yet)\n"
    if os.path.exists(out_path):
        old = open(out_path).read()
        if "## Reading" in old:
            reading = old[old.index("## Reading"):]
    with open(out_path, "w") as f:
        f.write("\n".join(text) + "\n\n" + reading)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ksteps", type=int, default=50)
    ap.add_argument("--only", default="default,freeze")
    ap.add_argument("--shapes", default="S-FB,S-DM")
    ap.add_argument("--label", default="this", help="the tree this run measures: 'this' or 'parent'")
    ap.add_argument("--report", nargs="+", metavar=("OUT.md", "LOG"), help="write the markdown tables from JSON-line logs and exit")
    args = ap.parse_args()
    if args.report:
        return report(args.report[0], args.report[1:])
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_freeze.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for part in args.only.split(","):
        for shape in args.shapes.split(","):
            if part == "default":
                measure(shape, dev, args, args.label)
            else:
                for freeze in (None, "entities", "relations"):
                    measure(shape, dev, args, args.label, freeze=freeze)


if __name__ == "__main__":
    main()
