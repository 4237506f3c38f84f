#!/usr/bin/env python3
"""Adam and gradient clipping on the token-encoded steps, on one GPU (profiles/encoder_optim.md holds the tables):

  tok-default   the S-OLP-tok step of bench_configs.py with default keywords (Adagrad, deferred decay) -- the line to compare
                between two commits: it uses nothing a commit before the keywords lacks
  tok           the same step with optimizer="adam", and with Adagrad under a binding and a non-binding grad_clip
  lstm          bench_lstm.py's S-OLP-lstm step, Adagrad against Adam
  sweep         okge_adam_multi on the token-pooled step's four tensors (two token tables with the maps a backward stamped, two
                batch-norm buffers) against the same update as two okge_adam_step calls without maps, and torch.optim.Adam(fused=True)

Every step figure is the median of `--windows` windows of `--steps` steps, each window closed by a device synchronise, with the
fastest and slowest window beside it; the sweep figures are device events around `--iters` calls.  One JSON object per line."""
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

from open_knowledge_graph_embeddings_amd import hotpath as H  # noqa: E402
import bench_configs  # noqa: E402


def windows(name, step, batches, args, **extra):
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
    out = {"workload": name, "ms_per_step_median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
           "windows": args.windows, "steps": args.steps, **extra}
    print(json.dumps(out), flush=True)
    return out


def tok_step(dev, **kw):
    """bench_configs.setup_s_olp_tok's tensors and batches under other keywords (the same seeds: the same problem)"""
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep
    rng = np.random.default_rng(1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)          # noqa: E731
    torch.manual_seed(1)
    step, batches = bench_configs.setup_s_olp_tok(dev, rng, t)[:2]
    if kw:
        step = TokenPooledTrainStep(step.entity, step.relation, "complex", lr=0.1, dropout=0.1, seed=1, **kw)
    return step, batches


def grad_norm(step, batch):
    step.forward_backward(batch)
    norm = float(torch.sqrt(sum((t[1].double() ** 2).sum() for t in step._param_groups())))
    step.optimizer_step()
    return norm


def tok_default(dev, args):
    step, batches = tok_step(dev)
    windows("S-OLP-tok default keywords", step, batches, args, decay_window=step.decay_window)


def tok(dev, args):
    for name, kw in (("adagrad (default)", {}), ("adam", dict(optimizer="adam")), ("adagrad, binding grad_clip", dict(grad_clip="binding")),
                     ("adagrad, grad_clip 1e6 (not binding)", dict(grad_clip=1e6)), ("adam, binding grad_clip", dict(optimizer="adam", grad_clip="binding"))):
        if kw.get("grad_clip") == "binding":
            probe, batches = tok_step(dev)
            kw = dict(kw, grad_clip=0.5 * grad_norm(probe, batches[0]))
            del probe, batches
            torch.cuda.empty_cache()
        step, batches = tok_step(dev, **kw)
        out = windows("S-OLP-tok " + name, step, batches, args, decay_window=step.decay_window, grad_clip=kw.get("grad_clip", 0.0))
        if step.grad_norm is not None:
            print(json.dumps({"workload": out["workload"], "last_grad_norm": float(step.grad_norm.item())}), flush=True)
        del step, batches
        torch.cuda.empty_cache()


def lstm(dev, args):
    import bench_lstm as BL
    from open_knowledge_graph_embeddings_amd.lstm import LSTMTrainStep
    for opt in ("adagrad", "adam"):
        rng = np.random.default_rng(7)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        n_ent, n_rel, vt_e, vt_r, d, B, N, L = BL.SHAPES["S-OLP-lstm"]
        torch.manual_seed(7)
        ent = BL.make_slot(rng, dev, vt_e, BL.make_token_matrix(rng, n_ent, vt_e, L), d)
        rel = BL.make_slot(rng, dev, vt_r, BL.make_token_matrix(rng, n_rel, vt_r, L), d)
        st = LSTMTrainStep(ent, rel, "complex", lr=0.1, dropout=0.1, seed=1, optimizer=opt)
        batches = [BL.positives_batch(rng, t, n_ent, n_rel, B, N, 1, cand_ids=t(rng.choice(n_ent - 2, N, replace=False).astype(np.int32) + 2))
                   for _ in range(2)]
        windows("S-OLP-lstm " + opt, st, batches, args)
        del st, ent, rel, batches
        torch.cuda.empty_cache()


def events(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / iters * 1e3, 2)          # us per call


def sweep(dev, args):
    step, batches = tok_step(dev, optimizer="adam")
    step.forward_backward(batches[0])                           # the maps as a backward leaves them
    eng = step.engine
    groups = step._param_groups()
    tensors = [(t[0], t[1]) + step._adam[t[0].data_ptr()] + tuple(t[3:5]) for t in groups]
    dense = [x[:5] for x in tensors]
    stamped = [float((t[5] == t[6]).float().mean()) for t in tensors[:2]]
    n = sum(t[0].numel() for t in tensors)
    out = {"tensors": [list(t[0].shape) for t in tensors], "floats": n, "stamped_row_share": [round(x, 4) for x in stamped], "iters": args.iters}
    params = [torch.nn.Parameter(t[0].clone()) for t in tensors]
    for q, t in zip(params, tensors):
        q.grad = torch.zeros_like(q)
    try:
        ref = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-10, fused=True)
    except (RuntimeError, ValueError, TypeError) as e:
        ref, out["torch_fused_us"] = None, f"not offered: {str(e).splitlines()[0][:80]}"
    for rep in range(2):                                        # alternating: the three see the same clock and the same neighbours
        out[f"adam_multi_us_rep{rep}"] = events(lambda: eng.adam_multi(tensors, 1e-3, (0.9, 0.999), 1e-8, 1e-10), args.iters)
        out[f"adam_step_pairs_us_rep{rep}"] = events(lambda: (eng.adam(dense[:2], 1e-3, (0.9, 0.999), 1e-8, 1e-10, zero_grad=1),
                                                              eng.adam(dense[2:], 1e-3, (0.9, 0.999), 1e-8, 1e-10, zero_grad=1)), args.iters)
        if ref is not None:
            out[f"torch_fused_us_rep{rep}"] = events(ref.step, args.iters)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", default="tok-default,tok,lstm,sweep")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_encoder_optim.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    for name in args.only.split(","):
        {"tok-default": tok_default, "tok": tok, "lstm": lstm, "sweep": sweep}[name](dev, args)


if __name__ == "__main__":
    main()
