#!/usr/bin/env python3
"""Top-k link prediction: the fused route (predict.TopKPredictor -> okge_topk_prefixes) against the route a caller had before
it: okge_score_prefixes into a (B, N) block, then torch.topk.  Where the block would exceed --block-gib the block route runs per
candidate range (block of one range -> torch.topk -> the per-range lists concatenated -> torch.topk over them).

Method: every shape is warmed up, then timed in windows of >= 0.25 s of back-to-back calls that end in a device synchronise;
the two routes alternate window by window and the MEDIAN window is reported.  The per-kernel split comes from a separate run
with the library's HIP-event timers on (okge_timing_*).  Needs an MI355X; writes a markdown table (stdout, or --out).

    python tools/bench_topk.py --out profiles/topk_measured.md
"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [  # name, scorer, d, B, N, k
    ("S-FB", "complex", 200, 512, 14541, 10),
    ("S-FB", "complex", 200, 512, 14541, 50),
    ("shard", "complex", 256, 4096, 312500, 10),
]


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block-gib", type=float, default=8.0, help="largest (B, N) score block the block route may allocate")
    ap.add_argument("--only", default=None, help="run only the shapes of this name")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk.py measures on an MI355X; there is no CPU path")
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath, PrefixBatch
    from open_knowledge_graph_embeddings_amd.predict import TopKPredictor
    dev = torch.device("cuda:0")
    hp = HotPath(dev)
    lines = ["| shape | scorer | d | B | N | k | fused ms | block ms | block / fused | block route | fused workspace | of it records | "
             "scores bit-equal | columns equal |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    splits = []
    for name, scorer, d, B, N, k in SHAPES:
        if args.only and name != args.only:
            continue
        g = torch.Generator(device="cpu").manual_seed(d + N)
        n_ent, n_rel = N + 2, 240
        E = (torch.randn((n_ent, d), generator=g) * 0.1).to(dev)
        R = (torch.randn((n_rel, d), generator=g) * 0.1).to(dev)
        ri = lambda hi, n: torch.randint(2, hi, (n,), generator=g, dtype=torch.int32).to(dev)      # noqa: E731
        ids = dict(po_rel=ri(n_rel, B // 2), po_obj=ri(n_ent, B // 2), sp_subj=ri(n_ent, B - B // 2), sp_rel=ri(n_rel, B - B // 2))
        batch = PrefixBatch(cand_first=2, n_cand=N, **ids)
        pred = TopKPredictor(E, R, scorer, k, engine=hp)

        # block route: whole block, or ranges of whole 64-candidate tiles under the cap
        cap_cols = int(args.block_gib * 2**30 / (4 * B)) // 64 * 64
        rn = N if N <= cap_cols else cap_cols
        n_ranges = math.ceil(N / rn)
        block = torch.empty((B, (rn + 3) // 4 * 4), dtype=torch.float32, device=dev)

        def block_route():
            parts_s, parts_c = [], []
            for r in range(n_ranges):
                lo, n = r * rn, min(rn, N - r * rn)
                hp.score(E, R, scorer, PrefixBatch(cand_first=2 + lo, n_cand=n, **ids), out=block[:, :n])
                s, c = torch.topk(block[:, :n], min(k, n), dim=1)
                parts_s.append(s)
                parts_c.append(c + lo)
            if n_ranges == 1:
                return parts_s[0], parts_c[0]
            s, j = torch.topk(torch.cat(parts_s, 1), k, dim=1)
            return s, torch.cat(parts_c, 1).gather(1, j)

        def fused_route():
            return pred.run(batch)

        for _ in range(args.warmup):
            fused_route()
            block_route()
        fs, _, fc = fused_route()
        bs, bc = block_route()
        torch.cuda.synchronize()
        bit_equal = bool(torch.equal(fs.view(torch.int32), bs.view(torch.int32)))
        cols_equal = float((fc.long() == bc.long()).float().mean())           # (torch.topk leaves the order of ties open)
        it_f = max(3, math.ceil(0.25 / window(fused_route, 3)))
        it_b = max(3, math.ceil(0.25 / window(block_route, 3)))
        tf, tb = [], []
        for _ in range(args.windows):
            tf.append(window(fused_route, it_f))
            tb.append(window(block_route, it_b))
        mf, mb = statistics.median(tf) * 1e3, statistics.median(tb) * 1e3
        ws = int(hp.lib.okge_topk_workspace_bytes(B, N, d, k, 0))
        rec = ws - int(hp.lib.okge_score_workspace_bytes(B, d))
        lines.append(f"| {name} | {scorer} | {d} | {B} | {N} | {k} | {mf:.3f} (min {min(tf) * 1e3:.3f}, max {max(tf) * 1e3:.3f}) | "
                     f"{mb:.3f} (min {min(tb) * 1e3:.3f}, max {max(tb) * 1e3:.3f}) | {mb / mf:.2f} | "
                     f"{'whole block' if n_ranges == 1 else f'{n_ranges} ranges of {rn}'}, {block.numel() * 4 / 2**20:.0f} MiB | "
                     f"{ws / 2**20:.1f} MiB | {rec / 2**20:.1f} MiB | {bit_equal} | {cols_equal:.6f} |")
        # per-kernel split, a run of its own
        for label, fn in (("fused", fused_route), ("block", block_route)):
            n_calls = max(3, it_f // 4 if label == "fused" else it_b // 4)
            hp.timing(True)
            for _ in range(n_calls):
                fn()
            torch.cuda.synchronize()
            t = hp.timing_collect()
            hp.timing(False)
            splits.append(f"- {name} k={k} {label}: " + ", ".join(f"`{kn}` {ms / n_calls:.4f} ms x {cnt // n_calls}" for kn, (ms, cnt) in sorted(t.items()))
                          + ("" if label == "fused" else "  (+ `torch.topk`, not a library kernel: block ms minus these)"))
        del block, E, R, pred
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n\nPer-kernel split (HIP events around every library launch, ms per call x launches per call):\n\n" + "\n".join(splits) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
