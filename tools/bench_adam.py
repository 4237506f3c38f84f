#!/usr/bin/env python3
"""Adam beside Adagrad on one GPU, same build, same run (profiles/adam.md holds one run's table):

  step    ms/step of FusedTrainStep at the S-FB shape (|E| = 14 543, d = 200, B = 512, 1-vs-all BCE) with optimizer="adam" and
          with the default Adagrad, alternating, with the library's per-kernel HIP-event averages
  sweep   okge_adam_step and okge_adagrad_step2 alone (zero_grad = 0) on two pairs of tensors -- S-FB's two tables, and a
          250 000 x 256 table beside a 1 000 x 256 one -- and torch.optim.Adam on the same tensors (foreach, and fused=True where
          this torch offers it).  Kernel time: HIP events around each launch (the library's timers); torch: events around the
          whole step() (its time includes the launches of the foreach chain).  Bytes: 4 n per stream -- Adam 7 streams (read p, g,
          m, v; write p, m, v), Adagrad 5 (read p, g, sum; write p, sum: with a fresh gradient every element changes).

Prints one JSON object per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from open_knowledge_graph_embeddings_amd import hotpath as H  # noqa: E402
from open_knowledge_graph_embeddings_amd import synthetic  # noqa: E402
from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep  # noqa: E402

from bench_configs import run  # noqa: E402  (tools/ is the script's directory)


def step_pair(dev, steps, warmup):
    w = synthetic.WORKLOADS["S-FB"]
    E, R = synthetic.make_tables(w, seed=1234)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    batches = []
    for i in range(4):
        hb = synthetic.make_batch(w, seed=1234 + i)
        batches.append(H.PrefixBatch(po_rel=t(hb["po_rel"]), po_obj=t(hb["po_obj"]), sp_subj=t(hb["sp_subj"]), sp_rel=t(hb["sp_rel"]),
                                     pos_row=t(hb["pos_row"]), pos_col=t(hb["pos_col"]), cand_first=2, n_cand=w.N))
    mk = {"adagrad": lambda: FusedTrainStep(t(E), t(R), w.scorer, lr=w.lr, input_dropout=w.input_dropout, seed=1),
          "adam": lambda: FusedTrainStep(t(E), t(R), w.scorer, lr=1e-3, weight_decay=1e-10, input_dropout=w.input_dropout, seed=1,
                                         optimizer="adam")}
    objs = {k: f() for k, f in mk.items()}
    for rep in range(3):                                   # alternating: both see the same clock and the same neighbours
        for name, s in objs.items():
            out = run(f"S-FB {name} rep{rep}", s, batches, steps=steps, warmup=warmup, quiet=True)
            print(json.dumps(out), flush=True)


def timed_kernel(eng, name, fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    eng.timing(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    per = eng.timing_collect()
    eng.timing(False)
    total, launches = per[name]
    return total / launches * 1e3                          # us per launch


def timed_torch(opt, iters):
    for _ in range(5):
        opt.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        opt.step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3                 # us per step


def sweeps(dev, iters):
    eng = H.HotPath(dev)
    for label, shapes in (("S-FB tables 14543x200 + 239x200", [(14543, 200), (239, 200)]),
                          ("250000x256 + 1000x256", [(250_000, 256), (1000, 256)])):
        n = sum(a * b for a, b in shapes)
        gen = torch.Generator(device=dev).manual_seed(1)
        mk = lambda scale=1.0: [torch.randn(sh, device=dev, generator=gen) * scale for sh in shapes]      # noqa: E731
        p, g = mk(0.1), mk(1e-3)
        m, v, s = mk(1e-3), [x.abs() for x in mk(1e-4)], [x.abs() for x in mk(1e-2)]
        states = [H.HotPath.adam_state(dev) for _ in shapes]
        out = {"tensors": label, "floats": n}
        for rep in range(3):
            us = timed_kernel(eng, "adam", lambda: eng.adam([(p[0], g[0], m[0], v[0], states[0]), (p[1], g[1], m[1], v[1], states[1])],
                                                            1e-3, (0.9, 0.999), 1e-8, 1e-10, zero_grad=0), iters)
            out[f"adam_us_rep{rep}"], out[f"adam_GBps_rep{rep}"] = round(us, 2), round(7 * 4 * n / us / 1e3, 1)
            us = timed_kernel(eng, "adagrad", lambda: eng.adagrad2(p[0], g[0], s[0], p[1], g[1], s[1], 1e-3, 1e-10, 1e-8, zero_grad=0), iters)
            out[f"adagrad_us_rep{rep}"], out[f"adagrad_GBps_rep{rep}"] = round(us, 2), round(5 * 4 * n / us / 1e3, 1)
        params = [torch.nn.Parameter(x.clone()) for x in p]
        for q, x in zip(params, g):
            q.grad = x.clone()
        for kind, kw in (("foreach", dict(foreach=True)), ("fused", dict(fused=True))):
            try:
                opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-10, **kw)
                us = timed_torch(opt, iters)
                out[f"torch_{kind}_us"], out[f"torch_{kind}_GBps"] = round(us, 2), round(7 * 4 * n / us / 1e3, 1)
            except (RuntimeError, ValueError, TypeError) as e:
                out[f"torch_{kind}_us"] = f"not offered: {str(e).splitlines()[0][:80]}"
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--only", choices=["step", "sweep"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    if args.only in (None, "sweep"):
        sweeps(dev, args.iters)
    if args.only in (None, "step"):
        step_pair(dev, args.steps, args.warmup)


if __name__ == "__main__":
    main()
