"""CPU-only: ShardedTopKPredictor's exchange protocol over gloo (shard ranges, global columns, the all-gather of the per-shard
lists, the merge) with a NumPy engine standing in for the HIP kernels.  Every rank must return exactly the unsharded
reference list -- including a world size at which one rank holds no candidates, and filter columns on the shard boundary."""
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import kge_oracle as ko

SCORER, N_REL, D, N_PO, N_SP, K = "complex", 7, 8, 5, 6, 10


def tables(n_ent):
    rng = np.random.default_rng(11)
    # entries from a small set: exact score ties across shards are common
    E = rng.choice(np.asarray([-0.5, 0.0, 0.5], np.float32), size=(n_ent, D))
    R = rng.choice(np.asarray([-0.5, 0.0, 0.5], np.float32), size=(N_REL, D))
    return E, R


def problem(n_ent, world):
    from open_knowledge_graph_embeddings_amd.sharded import shard_range
    rng = np.random.default_rng(n_ent)
    b = {"po_rel": rng.integers(2, N_REL, N_PO).astype(np.int32), "po_obj": rng.integers(2, n_ent, N_PO).astype(np.int32),
         "sp_subj": rng.integers(2, n_ent, N_SP).astype(np.int32), "sp_rel": rng.integers(2, N_REL, N_SP).astype(np.int32)}
    nc = n_ent - 2
    # global columns on either side of every shard boundary (column = entity id - 2), in every row's filter
    edge = sorted({c for r in range(world) for c in (shard_range(n_ent, world, r)[1] - 3, shard_range(n_ent, world, r)[1] - 2)
                   if 0 <= c < nc}) if nc > 10 else []
    rows = []
    for r in range(N_PO + N_SP):
        extra = rng.choice(nc, size=int(rng.integers(0, min(5, nc))), replace=False).tolist() if r % 3 else []
        rows.append(sorted(set(edge) | set(extra)))
    rows[1] = sorted(set(range(nc)) - {0, nc - 1})               # two eligible candidates: a padded row
    b["filt_ptr"] = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    b["filt_col"] = np.asarray([c for r in rows for c in r], np.int32)
    return b


def reference(n_ent, world):
    import topk_reference as tr
    E, R = tables(n_ent)
    b = problem(n_ent, world)
    kind = ko.KIND_NAMES[SCORER]
    x = np.concatenate([ko.score_prefix(kind, ko.DIR_PO, E[b["po_obj"]], R[b["po_rel"]], E[2:]),
                        ko.score_prefix(kind, ko.DIR_SP, E[b["sp_subj"]], R[b["sp_rel"]], E[2:])]).astype(np.float32)
    return tr.topk_rows(x, K, b["filt_ptr"], b["filt_col"], first_id=2)


def _worker(rank, world, port, outdir, n_ent):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import topk_reference as tr
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch
    from open_knowledge_graph_embeddings_amd.sharded import ShardedTopKPredictor, shard_range
    from shard_engine_cpu import OracleShardEngine

    class TopKEngine(OracleShardEngine):
        """the two top-k calls of HotPath on the oracle's local score block"""

        def topk_queries(self, E_local, R, scorer, Q, B, batch, shard, k, filt_ptr=None, filt_col=None, range_n=0):
            x = self._local_scores(E_local, Q, B, batch, shard)[3]
            fp, fc = (None, None) if filt_ptr is None else (filt_ptr.numpy(), filt_col.numpy())
            s, c, _ = tr.topk_rows(x, k, fp, fc, col0=shard.cand_col0)
            return torch.from_numpy(s), torch.from_numpy(c)

        def topk_merge(self, scores, cols):
            s, c = tr.merge_lists(scores.numpy(), cols.numpy())
            return torch.from_numpy(s), torch.from_numpy(c)

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=__import__("datetime").timedelta(minutes=5))
    E, R = tables(n_ent)
    lo, hi = shard_range(n_ent, world, rank)
    pred = ShardedTopKPredictor(torch.from_numpy(E[lo:hi].copy()), torch.from_numpy(R.copy()), SCORER, n_ent, K, engine=TopKEngine())
    b = problem(n_ent, world)
    t = torch.from_numpy
    batch = PrefixBatch(po_rel=t(b["po_rel"]), po_obj=t(b["po_obj"]), sp_subj=t(b["sp_subj"]), sp_rel=t(b["sp_rel"]))
    s, ids, c = pred.run(batch, t(b["filt_ptr"]), t(b["filt_col"]))
    np.savez(os.path.join(outdir, f"rank{rank}.npz"), s=s.numpy(), ids=ids.numpy(), c=c.numpy(), n_local=pred.n_cand_local)
    dist.destroy_process_group()


# (3, 5): shard ranges [0, 2) [2, 4) [4, 5) -- rank 0 holds only the two reserved ids, i.e. no candidate
@pytest.mark.parametrize("world,n_ent", [(2, 61), (3, 61), (3, 5)])
def test_sharded_topk_protocol_gloo(world, n_ent):
    import torch.multiprocessing as mp
    import topk_reference as tr
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as outdir:
        mp.spawn(_worker, args=(world, port, outdir, n_ent), nprocs=world, join=True)
        parts = [dict(np.load(os.path.join(outdir, f"rank{r}.npz"))) for r in range(world)]
    want = reference(n_ent, world)
    if n_ent == 5:
        assert int(parts[0]["n_local"]) == 0                    # the empty shard really occurred
    assert (want[1][1] == -1).sum() == K - 2 or n_ent == 5      # the padded row is padded
    for r, p in enumerate(parts):
        tr.assert_same((p["s"], p["c"], p["ids"]), want, f"rank {r}")
