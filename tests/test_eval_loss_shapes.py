"""The validation loss of the evaluation paths (okge_evaluate_fused_loss: one sweep, no (B, N) block; okge_evaluate_batch_loss:
reduced from the materialised block) at the shapes where the kernels take another path, against tests/eval_loss_reference.py
(float64) evaluated on the scores hp.score() writes -- existing code, bit-equal to what the sweep holds in registers.

Bound: 3e-5 relative, what tests/test_hip_parity.py holds the training loss to for the same bce_terms arithmetic; BCE relative
to L, KL relative to sum npos |lse| + sum |x_pos| (L is the difference of the two).  The same bound holds the new loss to
hp.forward_backward(loss_only=True) of the same batch and labels, and the fused to the materialising loss.  Equalities in
every case: ranks and the seven meters with the loss on are bit-equal to those with it off; a second run gives the same bits."""
import dataclasses

import numpy as np
import pytest
import torch

import eval_loss_reference as ref
from test_fused_eval import _case, _dev

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("production_config")]

TOL = 3e-5
MODES = (("bce", 0.0), ("bce", 0.1), ("kl", 0.0))


def _with_labels(batch, pos):
    """the batch with the rows' positives as (row, col) coordinates sorted by column: forward_backward's labels"""
    rows = np.concatenate([np.full(len(c), b, np.int64) for b, c in enumerate(pos)] + [np.zeros(0, np.int64)])
    cols = np.concatenate(list(pos) + [np.zeros(0, np.int64)])
    order = np.lexsort((rows, cols))
    return dataclasses.replace(batch, pos_row=_dev(rows[order].astype(np.int32)), pos_col=_dev(cols[order].astype(np.int32)))


def _triple(csr, B, col):
    """three more groups for the last row, every one naming `col` (once alone, twice beside another id)"""
    ids = np.concatenate([csr["ids"], np.asarray([col, col, 1, 0, col], np.int32)])
    grp = np.concatenate([csr["grp_ptr"], csr["grp_ptr"][-1] + np.asarray([1, 3, 5], np.int64)])
    row = csr["row_ptr"].copy()
    row[B] += 3
    return dict(csr, ids=ids, grp_ptr=grp, row_ptr=row)


def _no_groups(csr, B):
    return dict(csr, row_ptr=np.zeros(B + 1, np.int64), grp_ptr=np.zeros(1, np.int64), ids=np.zeros(0, np.int32))


def _check(hp, E, R, scorer, batch, csr, N, fused=True, what=""):
    Et, Rt = _dev(E), _dev(R)
    d = {k: _dev(v) for k, v in csr.items()}
    fc = d["filt_col"] if d["filt_col"].numel() else torch.zeros(1, dtype=torch.int32, device="cuda")
    B = batch.B
    x = hp.score(Et, Rt, scorer, batch).cpu().numpy().astype(np.float64)
    pos = ref.row_positives(csr["row_ptr"], csr["grp_ptr"], csr["ids"])
    labelled = _with_labels(batch, pos)
    n_groups = len(csr["grp_ptr"]) - 1
    args = (Et, Rt, scorer, batch, d["filt_ptr"], d["filt_col"], d["row_ptr"], d["grp_ptr"], d["ids"])
    if fused:
        r0, a0 = hp.evaluate_fused(*args)
        r0, a0 = r0.clone(), a0.clone()
    ld = (N + 3) // 4 * 4
    cur = torch.cuda.current_stream()
    out = {}
    for loss, eps in MODES:
        if loss == "bce":
            want = ref.bce_decomposed(x, pos, eps)
            scale = abs(want)
        else:
            want, scale = ref.kl_decomposed(x, pos), ref.kl_scale(x, pos)
        # the materialising path
        scores = torch.empty((B, ld), dtype=torch.float32, device="cuda")[:, :N]
        rk = torch.full((max(n_groups, 1),), -7, dtype=torch.int64, device="cuda")
        am = torch.zeros(7, dtype=torch.float64, device="cuda")
        Lm = hp.evaluate_batch(Et, Rt, scorer, batch, d["filt_ptr"], fc, d["row_ptr"], d["grp_ptr"], d["ids"], scores, rk, am, cur,
                               loss=loss, label_smoothing=eps)
        Lm2 = hp.evaluate_batch(Et, Rt, scorer, batch, d["filt_ptr"], fc, d["row_ptr"], d["grp_ptr"], d["ids"], scores, rk, am, cur,
                                loss=loss, label_smoothing=eps)
        Lt = hp.forward_backward(Et, Rt, scorer, labelled, None, None, loss=loss, label_smoothing=eps, loss_only=True)
        Lm, Lm2, Lt = Lm.item(), Lm2.item(), Lt.item()
        print(f"{what} {loss} eps={eps}: float64 {want!r} scale {scale!r} block {Lm!r} ({abs(Lm - want) / max(scale, 1e-300):.2e}) "
              f"train {Lt!r} ({abs(Lt - want) / max(scale, 1e-300):.2e})", end="")
        assert Lm == Lm2
        assert abs(Lm - want) <= TOL * scale, (what, loss, eps, "block", Lm, want)
        assert abs(Lm - Lt) <= TOL * scale, (what, loss, eps, "block vs train", Lm, Lt)
        if fused:
            r1, a1, L1 = hp.evaluate_fused(*args, loss=loss, label_smoothing=eps)
            r1, a1, L1 = r1.clone(), a1.clone(), L1.item()
            r2, a2, L2 = hp.evaluate_fused(*args, loss=loss, label_smoothing=eps)
            print(f" fused {L1!r} ({abs(L1 - want) / max(scale, 1e-300):.2e})", end="")
            assert torch.equal(r0, r1) and torch.equal(a0, a1), (what, loss, "ranks / meters moved with the loss on")
            assert torch.equal(r1, r2) and L2.item() == L1, (what, loss, "second run")
            assert torch.equal(rk[:n_groups], r0), (what, loss, "materialising ranks")
            assert abs(L1 - want) <= TOL * scale, (what, loss, eps, "fused", L1, want)
            assert abs(L1 - Lt) <= TOL * scale, (what, loss, eps, "fused vs train", L1, Lt)
            assert abs(L1 - Lm) <= TOL * scale, (what, loss, eps, "fused vs block", L1, Lm)
            out[(loss, eps)] = L1
        else:
            out[(loss, eps)] = Lm
        print()
        if n_groups == 0 and loss == "kl":
            assert want == 0.0 and Lm == 0.0 and out[(loss, eps)] == 0.0
    return out


# d (KB): 16 (4, "KB 1" padded), 200 (13), 256 (16), 258 / 512 (32: the 64k kernel, stream-K).  n_ent - 2 = N: 40 (one partial
# tile), 64, 65 .. 67 (a one-column tail), then several tiles.  B = 1, 33, 130; po-only and sp-only; candidate id lists.
CASES = [
    # d, scorer, n_ent, (n_po, n_sp), max_groups, ties, cand_list, many
    (16, "complex", 66, (1, 0), 3, False, False, None),
    (16, "distmult", 42, (13, 20), 2, False, False, None),
    (200, "complex", 67, (65, 65), 3, False, False, None),
    (200, "distmult", 68, (20, 13), 6, True, False, None),
    (256, "complex", 69, (100, 30), 2, True, False, None),
    (256, "distmult", 700, (0, 70), 3, False, False, None),
    (258, "distmult", 700, (70, 0), 3, False, False, None),
    (258, "complex", 67, (13, 20), 2, False, False, None),
    (512, "complex", 1500, (33, 31), 3, False, False, 1700),      # a chunk with more groups than the LDS counters hold
    (512, "distmult", 3000, (100, 30), 1, False, False, None),
    (512, "complex", 66, (1, 0), 2, True, False, None),
    (200, "complex", 900, (17, 16), 3, False, True, None),
    (512, "distmult", 515, (40, 25), 2, False, True, 70),
    (64, "distmult", 2050, (64, 64), 6, False, False, 70),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_eval_loss_shapes(okge_lib, i):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    d, scorer, n_ent, (n_po, n_sp), max_groups, ties, cand_list, many = CASES[i]
    rng = np.random.default_rng(4200 + i)
    E, R, batch, csr, N = _case(rng, n_ent, 30, d, n_po, n_sp, scorer, max_groups, ties, cand_list=cand_list, many=many)
    csr = _triple(csr, batch.B, min(7, N - 1))                   # the last row names one column three times
    _check(hp, E, R, scorer, batch, csr, N, what=f"case {i}")


@pytest.mark.parametrize("d,scorer", [(200, "complex"), (512, "distmult")])
def test_eval_loss_without_groups(okge_lib, d, scorer):
    """no row has an answer group: the KL loss is exactly 0, the BCE loss is the softplus sum; the batch is swept all the same"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(d)
    E, R, batch, csr, N = _case(rng, 300, 30, d, 20, 13, scorer, 2, False)
    out = _check(hp, E, R, scorer, batch, _no_groups(csr, batch.B), N, what=f"no groups d={d}")
    assert out[("kl", 0.0)] == 0.0 and out[("bce", 0.0)] > 0.0


@pytest.mark.parametrize("d,scorer", [(200, "complex"), (256, "distmult"), (512, "complex")])
def test_eval_loss_large_scores(okge_lib, d, scorer):
    """tables scaled so that |x| reaches 60 .. 90: softplus must not overflow, KL must subtract the row maximum"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(90 + d)
    E, R, batch, csr, N = _case(rng, 700, 30, d, 33, 31, scorer, 3, False)
    x = hp.score(_dev(E), _dev(R), scorer, batch)
    f = (75.0 / float(x.abs().max().item())) ** (1.0 / 3.0)      # the scorers are trilinear in the tables
    E, R = (E * np.float32(f)).astype(np.float32), (R * np.float32(f)).astype(np.float32)
    top = float(hp.score(_dev(E), _dev(R), scorer, batch).abs().max().item())
    assert 60.0 <= top <= 90.0, top
    _check(hp, E, R, scorer, batch, csr, N, what=f"large scores d={d}")


@pytest.mark.parametrize("d,scorer", [(32, "complex"), (200, "distmult")])
def test_eval_loss_tail_split(okge_lib, monkeypatch, d, scorer):
    """more candidate tiles than CUs (275 = 256 + 19, as test_fused_eval.py::test_tail_split_sweeps): the loss partials of the
    tail launch's (tile, row split) workgroups land where the plain launch puts them -- the same bits with OKGE_TAIL_SPLIT
    on and off"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(77 + d)
    E, R, batch, csr, N = _case(rng, 64 * 274 + 39, 30, d, 130, 126, scorer, max_groups=3, ties=False, many=70)
    assert (N + 63) // 64 == 275 and batch.B == 256
    got = {}
    for split in ("0", "1"):
        monkeypatch.setenv("OKGE_TAIL_SPLIT", split)
        got[split] = _check(hp, E, R, scorer, batch, csr, N, what=f"tail split {split} d={d}")
    assert got["0"] == got["1"]


def _batches(rng, n_ent, d, scorer, n, n_rel=20):
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    cbs, raw = [], []
    for k in range(n):
        _, _, batch, csr, N = _case(rng, n_ent, n_rel, d, 9 + 5 * (k % 4), 14 - 3 * (k % 5), scorer, 1 + k % 3, False, cand_list=k == 2)
        if k == 5:
            csr = _no_groups(csr, batch.B)                        # a batch without any answer group still has a loss
        dd = {kk: _dev(v) for kk, v in csr.items()}
        cbs.append(CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"],
                                 filt_ptr=dd["filt_ptr"], filt_col=dd["filt_col"]))
        raw.append((batch, csr, dd, N))
    return cbs, raw


@pytest.mark.parametrize("loss,eps", MODES)
def test_fused_evaluator_loss(okge_lib, loss, eps):
    """FusedEvaluator(loss=...): n_streams 1 / 2 / 3 and run_len 1 / 7 over twelve small batches give bit-identical
    batch_losses and meter, equal to single evaluate_fused calls; the meter is sum L / sum B N with count sum B N; the other
    meters and the ranks are those of a loss=None run, which leaves the loss meter empty; PipelinedEvaluator agrees within the
    bound"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    rng = np.random.default_rng(31)
    n_ent, d, scorer = 500, 200, "complex"
    E = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32)
    R = (rng.standard_normal((20, d)) * 0.3).astype(np.float32)
    Et, Rt = _dev(E), _dev(R)
    cbs, raw = _batches(rng, n_ent, d, scorer, 12)
    hp = H.HotPath(Et.device)
    single, want, scale, elems = [], [], [], 0
    for batch, csr, dd, N in raw:
        _, _, L = hp.evaluate_fused(Et, Rt, scorer, batch, dd["filt_ptr"], dd["filt_col"], dd["row_ptr"], dd["grp_ptr"], dd["ids"],
                                    loss=loss, label_smoothing=eps)
        single.append(L.item())
        x = hp.score(Et, Rt, scorer, batch).cpu().numpy().astype(np.float64)
        pos = ref.row_positives(csr["row_ptr"], csr["grp_ptr"], csr["ids"])
        want.append(ref.bce_decomposed(x, pos, eps) if loss == "bce" else ref.kl_decomposed(x, pos))
        scale.append(abs(want[-1]) if loss == "bce" else ref.kl_scale(x, pos))
        elems += batch.B * N
    for got, w, s in zip(single, want, scale):
        assert abs(got - w) <= TOL * s, (got, w)
    base = FusedEvaluator(Et, Rt, scorer, collect_ranks=True)
    res0, n0 = base.run(iter(cbs))
    assert res0["loss"].count == 0 and base.batch_losses is None
    total = 0.0
    for v in single:
        total += v
    for n_streams in (1, 2, 3):
        for run_len in (1, 7):
            ev = FusedEvaluator(Et, Rt, scorer, n_streams=n_streams, run_len=run_len, collect_ranks=True, loss=loss, label_smoothing=eps)
            for _ in range(2):                                    # (a second pass through the same object, buffers reused)
                res, n = ev.run(iter(cbs))
                assert n == n0 and torch.equal(ev.ranks, base.ranks)
                assert ev.batch_losses.dtype == torch.float64 and ev.batch_losses.cpu().tolist() == single, (n_streams, run_len)
                assert res["loss"].count == elems and res["loss"].avg == total / elems
                for k in ("mrr", "mr", "h1", "h3", "h10", "h50"):
                    assert res[k].avg == res0[k].avg and res[k].count == res0[k].count, k
    pe = PipelinedEvaluator(Et, Rt, scorer, collect_ranks=True, loss=loss, label_smoothing=eps)
    res, n = pe.run(iter(cbs))
    assert n == n0 and torch.equal(pe.ranks, base.ranks) and res["loss"].count == elems
    for got, w, s in zip(pe.batch_losses.cpu().tolist(), want, scale):
        assert abs(got - w) <= TOL * s, (got, w)
    # (without a loss the materialising path has nothing to launch for a batch without groups and refuses it)
    assert PipelinedEvaluator(Et, Rt, scorer).run(cb for k, cb in enumerate(cbs) if k != 5)[0]["loss"].count == 0


def test_pipelined_evaluator_loss_wide(okge_lib):
    """d = 520, |E| = 300: above the fused evaluation's slot sizes, the materialising path alone; FusedEvaluator keeps refusing
    at construction"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    hp = H.HotPath("cuda:0")
    rng = np.random.default_rng(520)
    E, R, batch, csr, N = _case(rng, 300, 30, 520, 20, 13, "complex", 3, False)
    csr = _triple(csr, batch.B, 7)
    want = _check(hp, E, R, "complex", batch, csr, N, fused=False, what="wide d=520")
    Et, Rt = _dev(E), _dev(R)
    dd = {k: _dev(v) for k, v in csr.items()}
    cb = CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"], filt_ptr=dd["filt_ptr"],
                       filt_col=dd["filt_col"])
    for loss, eps in MODES:
        ev = PipelinedEvaluator(Et, Rt, "complex", loss=loss, label_smoothing=eps)
        res, _ = ev.run([cb, cb])
        assert ev.batch_losses.cpu().tolist() == [want[(loss, eps)]] * 2
        assert res["loss"].count == 2 * batch.B * N
        assert res["loss"].avg == (want[(loss, eps)] + want[(loss, eps)]) / (2 * batch.B * N)
    with pytest.raises(NotImplementedError, match="PipelinedEvaluator"):
        FusedEvaluator(Et, Rt, "complex", loss="bce")


def test_evaluator_loss_keyword_refusals(okge_lib):
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    E, R = torch.zeros((10, 8), device="cuda"), torch.zeros((4, 8), device="cuda")
    for cls in (FusedEvaluator, PipelinedEvaluator):
        with pytest.raises(ValueError, match="unknown loss"):
            cls(E, R, "complex", loss="mse")
        with pytest.raises(NotImplementedError, match="no validation loss"):
            cls(E, R, "tucker3", loss="bce")
