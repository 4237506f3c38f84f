"""Fused evaluation (okge_evaluate_fused: point scores + tile sweep with in-register counting + ranks, no (B, N) score
block) against the materialising path (okge_score_prefixes + okge_filtered_ranks) and the oracle's rank rule
(openkge/dataset.py:423-453).  The bar: ranks BIT-EQUAL -- the point scores reproduce the tile kernel's fp32 summation
order exactly, so not even a near-tie may move -- and the same meters."""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import kge_oracle as ko

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("production_config")]   # OKGE_VALIDATE off, like production


def _dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).cuda()


def _case(rng, n_ent, n_rel, d, n_po, n_sp, scorer, max_groups, ties, cand_list=False, many=None):
    """random tables / prefixes, answer groups (multi-id groups, rows without groups, one row with `many` groups) and an
    all-splits filter; `ties`: tables from a tiny alphabet so that many scores are exactly equal"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    if ties:
        E = rng.integers(-1, 2, (n_ent, d)).astype(np.float32) * 0.5
        R = rng.integers(-1, 2, (n_rel, d)).astype(np.float32) * 0.5
    else:
        E = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32)
        R = (rng.standard_normal((n_rel, d)) * 0.3).astype(np.float32)
    batch = H.PrefixBatch()
    if n_po:
        batch.po_rel, batch.po_obj = _dev(rng.integers(2, n_rel, n_po).astype(np.int32)), _dev(rng.integers(2, n_ent, n_po).astype(np.int32))
    if n_sp:
        batch.sp_subj, batch.sp_rel = _dev(rng.integers(2, n_ent, n_sp).astype(np.int32)), _dev(rng.integers(2, n_rel, n_sp).astype(np.int32))
    if cand_list:
        cand = rng.permutation(np.arange(2, n_ent))[:max(8, (n_ent - 2) // 3)].astype(np.int32)
        batch.cand_ids, N = _dev(cand), len(cand)
    else:
        batch.cand_first, batch.n_cand, N = 2, n_ent - 2, n_ent - 2
    B = n_po + n_sp
    row_ptr, grp_ptr, ids, filt_ptr, filt_col = [0], [0], [], [0], []
    for b in range(B):
        ng = 0 if rng.random() < 0.1 else int(rng.integers(1, max_groups + 1))
        if many is not None and b == B // 2:
            ng = many
        row_ids = []
        for _ in range(ng):
            g = rng.integers(0, N, int(rng.integers(1, 4))).tolist()
            ids.extend(g)
            row_ids.extend(g)
            grp_ptr.append(len(ids))
        row_ptr.append(len(grp_ptr) - 1)
        nf = int(rng.integers(0, 12)) if b != B // 3 else 300
        f = np.unique(np.concatenate([rng.integers(0, N, nf), np.asarray(row_ids, np.int64)])).astype(np.int64) if (nf or row_ids) else np.zeros(0, np.int64)
        if rng.random() < 0.2:
            f = f[: len(f) // 2]                  # not every answer is filtered (the reference filters what it is given)
        filt_col.extend(f.tolist())
        filt_ptr.append(len(filt_col))
    csr = dict(filt_ptr=np.asarray(filt_ptr, np.int64), filt_col=np.asarray(filt_col, np.int32), row_ptr=np.asarray(row_ptr, np.int64),
               grp_ptr=np.asarray(grp_ptr, np.int64), ids=np.asarray(ids, np.int32))
    return E, R, batch, csr, N


def _check(hp, E, R, scorer, batch, csr, N):
    Et, Rt = _dev(E), _dev(R)
    d = {k: _dev(v) for k, v in csr.items()}
    if d["filt_col"].numel() == 0:
        d["filt_col"] = torch.zeros(1, dtype=torch.int32, device="cuda")[:0]
    x = hp.score(Et, Rt, scorer, batch)
    ref = hp.filtered_ranks(x.contiguous(), d["filt_ptr"], d["filt_col"] if d["filt_col"].numel() else torch.zeros(1, dtype=torch.int32, device="cuda"),
                            d["row_ptr"], d["grp_ptr"], d["ids"]).cpu().numpy()
    acc_ref = torch.zeros(7, dtype=torch.float64, device="cuda")
    n_groups = len(csr["grp_ptr"]) - 1
    if n_groups:
        hp.rank_metrics(torch.from_numpy(ref).cuda(), acc_ref)
    ranks, acc = hp.evaluate_fused(Et, Rt, scorer, batch, d["filt_ptr"], d["filt_col"], d["row_ptr"], d["grp_ptr"], d["ids"])
    torch.cuda.synchronize()
    np.testing.assert_array_equal(ranks.cpu().numpy(), ref)
    np.testing.assert_allclose(acc.cpu().numpy(), acc_ref.cpu().numpy(), rtol=1e-12, atol=0)
    # and the oracle's rule on the same scores
    filt = np.zeros((batch.B, N), bool)
    for b in range(batch.B):
        filt[b, csr["filt_col"][csr["filt_ptr"][b]:csr["filt_ptr"][b + 1]]] = True
    np.testing.assert_array_equal(ref, ko.filtered_ranks(x.cpu().numpy(), filt, csr["row_ptr"], csr["grp_ptr"], csr["ids"]))
    return ranks


@pytest.mark.parametrize("i", range(16))
def test_fused_eval_random(okge_lib, i):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(1000 + i)
    scorer = "complex" if i % 2 == 0 else "distmult"
    d = [200, 64, 256, 24, 130, 208, 16, 100][i % 8]
    if scorer == "complex" and d % 2:
        d += 1
    n_ent = [700, 130, 3000, 67, 1500, 515, 66, 2050][i % 8]
    n_po, n_sp = [(40, 40), (0, 70), (100, 0), (13, 9), (64, 64), (1, 0), (33, 31), (130, 65)][i % 8]
    E, R, batch, csr, N = _case(rng, n_ent, 30, d, n_po, n_sp, scorer, max_groups=[2, 6, 1, 3][i % 4], ties=i % 3 == 0,
                                cand_list=i % 5 == 1, many=70 if i % 4 == 2 else None)
    _check(hp, E, R, scorer, batch, csr, N)


@pytest.mark.parametrize("i", range(10))
def test_fused_eval_wide_slots(okge_lib, i):
    """slot sizes 257 .. 512 (round 4): the counting mode of the register-tile kernel (fused_tile64k_kernel<count>, stream-K
    launch, operands swapped) + point scores in that kernel's two-half summation order -- ranks bit-equal to the materialising
    path, incl. chunks with more groups than the LDS counters hold (the take-turns path), ties, rows without groups, id lists"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(7000 + i)
    scorer = "complex" if i % 2 == 0 else "distmult"
    d = [512, 260, 320, 512, 400, 384, 258, 512, 448, 300][i]
    n_ent = [2100, 700, 130, 9000, 515, 3000, 67, 1500, 2050, 700][i]
    n_po, n_sp = [(64, 64), (40, 40), (0, 70), (256, 256), (13, 9), (100, 0), (1, 0), (33, 31), (130, 65), (20, 50)][i]
    # i == 3: the cfg3 shape of the table (d = 512, B = 512); i == 7: one row with 1700 groups: its chunk overflows the LDS counters
    E, R, batch, csr, N = _case(rng, n_ent, 30, d, n_po, n_sp, scorer, max_groups=[2, 6, 1, 3][i % 4], ties=i % 3 == 0,
                                cand_list=i % 5 == 1, many=1700 if i == 7 else (70 if i % 4 == 2 else None))
    _check(hp, E, R, scorer, batch, csr, N)


def test_fused_eval_fb15k237_batch(okge_lib):
    """the real FB15k-237 evaluation batch G10 at the BASELINE size, against the reference's own ranks"""
    from test_fb15k237_batch import check_ranks, tables
    from open_knowledge_graph_embeddings_amd import hotpath as H
    z = golden("g10_fb15k237_batch")
    _, E, R = tables(z)
    hp = H.HotPath("cuda:0")
    N = E.shape[0] - 2
    batch = H.PrefixBatch(po_rel=_dev(z["po_rel"].reshape(-1)), po_obj=_dev(z["po_obj"].reshape(-1)),
                          sp_subj=_dev(z["sp_subj"].reshape(-1)), sp_rel=_dev(z["sp_rel"].reshape(-1)), cand_first=2, n_cand=N)
    f = z["filter"]
    csr = dict(filt_ptr=np.concatenate([[0], np.cumsum(np.bincount(f[:, 0], minlength=512))]).astype(np.int64),
               filt_col=f[:, 1].astype(np.int32), row_ptr=z["row_ptr"], grp_ptr=z["grp_ptr"], ids=z["ids"])
    ranks = _check(hp, E, R, "complex", batch, csr, N)
    check_ranks(ranks.cpu().numpy(), z)


def test_fused_evaluator_equals_pipelined(okge_lib):
    """evaluate.FusedEvaluator over several batches of different shapes == evaluate.PipelinedEvaluator"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    rng = np.random.default_rng(5)
    n_ent, d = 900, 200
    E = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32)
    R = (rng.standard_normal((20, d)) * 0.3).astype(np.float32)
    cbs = []
    for k in range(5):
        _, _, batch, csr, N = _case(rng, n_ent, 20, d, 30 + 7 * k, 20 + 3 * k, "complex", 3, False, cand_list=k == 2)
        dd = {kk: _dev(v) for kk, v in csr.items()}
        cbs.append(CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"],
                                 filt_ptr=dd["filt_ptr"], filt_col=dd["filt_col"]))
    Et, Rt = _dev(E), _dev(R)
    a, na = FusedEvaluator(Et, Rt, "complex").run(cbs)
    b, nb = PipelinedEvaluator(Et, Rt, "complex").run(cbs)
    assert na == nb and na > 0
    for k in ("mrr", "mr", "h1", "h3", "h10", "h50"):
        assert abs(a[k].avg - b[k].avg) <= 1e-12 * max(1.0, abs(b[k].avg)), k
    for run_len in (1, 2):                                     # run boundaries: 5 batches as 1+1+1+1+1 and 2+2+1
        c, nc = FusedEvaluator(Et, Rt, "complex", run_len=run_len, two_streams=run_len == 2).run(iter(cbs))
        assert nc == na
        for k in ("mrr", "mr", "h1", "h3", "h10", "h50"):
            assert c[k].avg == a[k].avg, (run_len, k)


def test_fused_batches_ranks_equal_single_calls(okge_lib):
    """okge_evaluate_fused_batches with every batch's ranks kept (rank_offset = prefix sum of the group counts) ==
    okge_evaluate_fused batch by batch, bit for bit; refusals happen before the first launch"""
    import ctypes
    import torch
    from open_knowledge_graph_embeddings_amd import _native as NV
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator
    rng = np.random.default_rng(11)
    n_ent, d = 1500, 64
    E = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32)
    R = (rng.standard_normal((12, d)) * 0.3).astype(np.float32)
    Et, Rt = _dev(E), _dev(R)
    hp = H.HotPath(Et.device)
    cbs, want = [], []
    for k in range(7):
        _, _, batch, csr, N = _case(rng, n_ent, 12, d, 11 + 9 * k, 40 - 5 * k, "complex", 2 + k % 3, False, cand_list=k == 4)
        dd = {kk: _dev(v) for kk, v in csr.items()}
        cbs.append(CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"],
                                 filt_ptr=dd["filt_ptr"], filt_col=dd["filt_col"]))
        r, _ = hp.evaluate_fused(Et, Rt, "complex", batch, dd["filt_ptr"], dd["filt_col"], dd["row_ptr"], dd["grp_ptr"], dd["ids"])
        want.append(r.cpu().numpy().copy())
    fe = FusedEvaluator(Et, Rt, "complex", engine=hp, run_len=len(cbs))
    need, off, keep = 0, 0, []
    for i, cb in enumerate(cbs):
        nd, ng, ka = fe._fill(i, cb)
        keep.append(ka)
        need = max(need, nd)
        fe._arr[i].rank_offset = off
        off += ng
    slot = (need + 255) // 256 * 256
    ws = torch.empty(6 * slot, dtype=torch.uint8, device=Et.device)
    ranks = torch.full((off,), -7, dtype=torch.int64, device=Et.device)
    acc = torch.zeros(7, dtype=torch.float64, device=Et.device)
    main = torch.cuda.current_stream(Et.device).cuda_stream
    extra = [torch.cuda.Stream(device=Et.device) for _ in range(2)]
    args = (ctypes.byref(fe._t), fe._arr, len(cbs), ranks.data_ptr(), acc.data_ptr(), ws.data_ptr())
    def streams(k):
        return (ctypes.c_void_p * k)(main, *[x.cuda_stream for x in extra[:k - 1]]), k
    for k in (1, 2, 3):                                                  # one stream; two / three independent chains
        ranks.fill_(-7)
        acc.zero_()
        torch.cuda.synchronize()
        NV.check(hp.lib.okge_evaluate_fused_batches(*args, ws.numel(), *streams(k)), "okge_evaluate_fused_batches")
        torch.cuda.synchronize()
        assert np.array_equal(ranks.cpu().numpy(), np.concatenate(want))
        assert int(acc[0].item()) == off
    # too small a workspace: refused before the first launch, nothing written
    ranks.fill_(-7)
    assert hp.lib.okge_evaluate_fused_batches(*args, 3 * slot, *streams(2)) != 0
    assert hp.lib.okge_evaluate_fused_batches(*args, ws.numel(), (ctypes.c_void_p * 2)(main, main), 2) != 0    # the same stream twice
    torch.cuda.synchronize()
    assert int((ranks != -7).sum().item()) == 0


def test_fused_run_with_empty_and_one_direction_batches(okge_lib):
    """a run whose batches include one without any answer group (nothing to launch: it drops out of its chain), one with
    po rows only and one with sp rows only: meters equal the materialising evaluator's"""
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    rng = np.random.default_rng(23)
    n_ent, d = 700, 128
    E = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32)
    R = (rng.standard_normal((15, d)) * 0.3).astype(np.float32)
    Et, Rt = _dev(E), _dev(R)
    cbs = []
    for k, (n_po, n_sp) in enumerate(((20, 20), (0, 33), (17, 9), (41, 0), (8, 8), (12, 30))):
        _, _, batch, csr, N = _case(rng, n_ent, 15, d, n_po, n_sp, "complex", 3, False)
        if k in (2, 4):                                   # no answer groups at all in this batch
            B = n_po + n_sp
            csr = dict(csr, row_ptr=np.zeros(B + 1, np.int64), grp_ptr=np.zeros(1, np.int64), ids=np.zeros(0, np.int32))
        dd = {kk: _dev(v) for kk, v in csr.items()}
        cbs.append(CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"],
                                 filt_ptr=dd["filt_ptr"], filt_col=dd["filt_col"]))
    b, nb = PipelinedEvaluator(Et, Rt, "complex").run([cb for k, cb in enumerate(cbs) if k not in (2, 4)])
    for two in (True, False):
        a, na = FusedEvaluator(Et, Rt, "complex", run_len=8, two_streams=two).run(cbs)
        assert na == nb and na > 0
        for k in ("mrr", "mr", "h1", "h3", "h10", "h50"):
            assert abs(a[k].avg - b[k].avg) <= 1e-12 * max(1.0, abs(b[k].avg)), (two, k)


def test_evaluator_chain_counts_agree(okge_lib):
    """1 to 4 independent chains (FusedEvaluator) and 1 or 3 chains (PipelinedEvaluator) give the same meters; the C entry
    refuses 0 and 5 streams"""
    import ctypes
    import torch
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    rng = np.random.default_rng(31)
    n_ent, d = 1100, 96
    E = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32)
    R = (rng.standard_normal((9, d)) * 0.3).astype(np.float32)
    Et, Rt = _dev(E), _dev(R)
    cbs = []
    for k in range(11):
        _, _, batch, csr, N = _case(rng, n_ent, 9, d, 13 + 5 * k, 37 - 3 * k, "complex", 2 + k % 2, False, cand_list=k == 7)
        dd = {kk: _dev(v) for kk, v in csr.items()}
        cbs.append(CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"],
                                 filt_ptr=dd["filt_ptr"], filt_col=dd["filt_col"]))
    ref, n_ref = PipelinedEvaluator(Et, Rt, "complex", n_streams=1).run(cbs)
    runs = [FusedEvaluator(Et, Rt, "complex", n_streams=k, run_len=5).run(cbs) for k in (1, 2, 3, 4)]
    runs.append(PipelinedEvaluator(Et, Rt, "complex", n_streams=3).run(cbs))
    for res, n in runs:
        assert n == n_ref
        for key in ("mrr", "mr", "h1", "h3", "h10", "h50"):
            assert abs(res[key].avg - ref[key].avg) <= 1e-12 * max(1.0, abs(ref[key].avg)), key
    fe = FusedEvaluator(Et, Rt, "complex", n_streams=1, run_len=2)
    fe._fill(0, cbs[0])
    fe._arr[0].rank_offset = 0
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=Et.device)
    rk = torch.empty(4096, dtype=torch.int64, device=Et.device)
    acc = torch.zeros(7, dtype=torch.float64, device=Et.device)
    h = (ctypes.c_void_p * 5)(*[torch.cuda.current_stream(Et.device).cuda_stream] * 5)
    for bad in (0, 5):
        assert fe.engine.lib.okge_evaluate_fused_batches(ctypes.byref(fe._t), fe._arr, 1, rk.data_ptr(), acc.data_ptr(), ws.data_ptr(),
                                                         ws.numel(), h, bad) != 0


def test_pipelined_evaluator_many_small_batches_lose_no_group(okge_lib):
    """three unordered chains, 240 small batches (meter launches overlap across chains all the time): every answer group
    must be counted -- the meters of a chain go into that chain's own row and rank_metrics_kernel adds atomically -- and
    the result is identical from run to run"""
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    from open_knowledge_graph_embeddings_amd.evaluate import PipelinedEvaluator
    rng = np.random.default_rng(77)
    n_ent, d = 300, 32
    E = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32)
    R = (rng.standard_normal((7, d)) * 0.3).astype(np.float32)
    Et, Rt = _dev(E), _dev(R)
    cbs, total = [], 0
    for k in range(24):
        _, _, batch, csr, N = _case(rng, n_ent, 7, d, 3 + k % 5, 2 + k % 3, "complex", 3, False)
        dd = {kk: _dev(v) for kk, v in csr.items()}
        total += len(csr["grp_ptr"]) - 1
        cbs.append(CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"],
                                 filt_ptr=dd["filt_ptr"], filt_col=dd["filt_col"]))
    ref, n_ref = PipelinedEvaluator(Et, Rt, "complex", n_streams=1).run(cbs * 10)
    assert n_ref == 10 * total
    ev = PipelinedEvaluator(Et, Rt, "complex", n_streams=3)
    seen = []
    for _ in range(5):
        res, n = ev.run(cbs * 10)
        assert n == 10 * total                                   # exact: a lost update would drop a whole batch's groups
        for key in ("mr", "h1", "h3", "h10", "h50"):
            assert res[key].avg == ref[key].avg, key              # integer-valued sums: order cannot matter
        assert abs(res["mrr"].avg - ref["mrr"].avg) <= 1e-13
        seen.append(res["mrr"].avg)
    assert len(set(seen)) == 1                                   # per-chain rows summed in a fixed order: reproducible


@pytest.mark.parametrize("d,scorer", [(32, "complex"), (200, "distmult"), (256, "complex")])
def test_tail_split_sweeps(okge_lib, monkeypatch, d, scorer):
    """more candidate tiles than CUs (275 = 256 + 19): the score sweep and the counting sweep launch the leftover tiles apart,
    rows split across workgroups (okge_plan.h plan_sweep) -- rows are independent, so scores and ranks are BIT-EQUAL to the
    plain launch (OKGE_TAIL_SPLIT=0), and both equal the materialising path and the oracle's rank rule"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(77 + d)
    E, R, batch, csr, N = _case(rng, 64 * 274 + 39, 30, d, 130, 126, scorer, max_groups=3, ties=False, many=70)
    assert (N + 63) // 64 == 275 and batch.B == 256
    got = {}
    for split in ("0", "1"):
        monkeypatch.setenv("OKGE_TAIL_SPLIT", split)
        x = hp.score(_dev(E), _dev(R), scorer, batch).clone()
        got[split] = (x, _check(hp, E, R, scorer, batch, csr, N).clone())
    assert torch.equal(got["0"][0], got["1"][0])
    assert torch.equal(got["0"][1], got["1"][1])
