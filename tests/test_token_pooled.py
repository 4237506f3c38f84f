"""Token-pooled embedder on the GPU against vectors produced by the reference's
UnigramPoolingComplexRelationModel + AddLossModule (tests/golden/g9_unigram_*.npz) and against the oracle."""
import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from oracle import kge_oracle as ko

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def slots(z):
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenSlot
    bn = str(z["normalize"]) == "batchnorm"
    e = TokenSlot(dev(z["We"]), dev(z["ent_tokens"]), str(z["pool"]), bn, dev(z["bn_e_w"]) if bn else None, dev(z["bn_e_b"]) if bn else None)
    r = TokenSlot(dev(z["Wr"]), dev(z["rel_tokens"]), str(z["pool"]), bn, dev(z["bn_r_w"]) if bn else None, dev(z["bn_r_b"]) if bn else None)
    return e, r, bn


def batch_of(z):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    b = PrefixBatch()
    if "po_rel" in z.files:
        b.po_rel, b.po_obj = dev(z["po_rel"].reshape(-1)), dev(z["po_obj"].reshape(-1))
    if "sp_subj" in z.files:
        b.sp_subj, b.sp_rel = dev(z["sp_subj"].reshape(-1)), dev(z["sp_rel"].reshape(-1))
    b.cand_ids = dev(z["cand"].reshape(-1).astype(np.int32))
    b.pos_row, b.pos_col = positives_from_dense(dev(z["labels"]))
    return b


@pytest.mark.parametrize("name", [n for n in golden_names("g9_unigram_") if "_init_" not in n])
def test_train_forward_backward_matches_reference(okge_lib, name):
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep
    z = golden(name)
    e, r, bn = slots(z)
    st = TokenPooledTrainStep(e, r, "complex", lr=0.1)
    B, N = z["labels"].shape
    scores = torch.empty((B, (N + 3) // 4 * 4), device="cuda:0")[:, :N]
    loss = st.forward_backward(batch_of(z), scores=scores)
    torch.cuda.synchronize()
    np.testing.assert_allclose(scores.cpu().numpy(), z["outputs"], rtol=0, atol=1e-4)
    assert abs(float(loss[0]) - float(z["loss"])) <= 3e-5 * abs(float(z["loss"]))
    for mine, key in ((e.dW, "dWe"), (r.dW, "dWr")):
        np.testing.assert_allclose(mine.cpu().numpy(), z[key], rtol=0, atol=5e-5 * np.abs(z[key]).max())
    assert float(e.dW[0].abs().sum()) == 0 and float(r.dW[0].abs().sum()) == 0          # padding_idx row: no gradient
    if bn:
        d = e.d
        for sl, w in ((e, "e"), (r, "r")):
            np.testing.assert_allclose(sl.d_bn[:d].cpu().numpy(), z[f"d_bn_{w}_w"], rtol=0, atol=5e-5 * np.abs(z[f"d_bn_{w}_w"]).max())
            np.testing.assert_allclose(sl.d_bn[d:].cpu().numpy(), z[f"d_bn_{w}_b"], rtol=0, atol=5e-5 * np.abs(z[f"d_bn_{w}_b"]).max() + 1e-8)
            np.testing.assert_allclose(sl.running_mean.cpu().numpy(), z[f"run_{w}_mean"], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(sl.running_var.cpu().numpy(), z[f"run_{w}_var"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", [n for n in golden_names("g9_unigram_") if "_init_" not in n])
@torch.no_grad()                           # the reference's evaluation (trainer.py:366); with gradients: test_autograd_surface.py
def test_model_api_eval_tables_and_scores(okge_lib, name):
    """precompute_embeddings_from_tokens + sp/po_prefix_score in eval mode, after the training step's running-stat
    update (the fixture's eval outputs were taken after one training forward)."""
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.token_pooled import UnigramPoolingComplexRelationModel
    z = golden(name)
    n_ent, L = z["ent_tokens"].shape
    n_rel = z["rel_tokens"].shape[0]
    md = EntityRelationDatasetMeta(entities_size=n_ent, relations_size=n_rel, entity_tokens_size=z["We"].shape[0],
                                   relation_tokens_size=z["Wr"].shape[0], max_length=(L, L),
                                   entity_id_to_tokens_map=[[int(t) for t in row if t] or [0] for row in z["ent_tokens"]],
                                   relation_id_to_tokens_map=[[int(t) for t in row if t] or [0] for row in z["rel_tokens"]])
    bn = str(z["normalize"]) == "batchnorm"
    m = UnigramPoolingComplexRelationModel(entity_slot_size=z["We"].shape[1], relation_slot_size=z["We"].shape[1], train_data=md,
                                           pool=str(z["pool"]), normalize="batchnorm" if bn else None, dropout=0.0, init_std=0.3)
    np.testing.assert_array_equal(m.entity_token_ids.numpy(), z["ent_tokens"])
    m = m.cuda()
    m.entity_embedding.weight.data.copy_(dev(z["We"]))
    m.relation_embedding.weight.data.copy_(dev(z["Wr"]))
    if bn:
        for mod, w in ((m.entity_batchnorm, "e"), (m.relation_batchnorm, "r")):
            mod.weight.data.copy_(dev(z[f"bn_{w}_w"]))
            mod.bias.data.copy_(dev(z[f"bn_{w}_b"]))
            mod.running_mean.copy_(dev(z[f"run_{w}_mean"]))
            mod.running_var.copy_(dev(z[f"run_{w}_var"]))
    m.eval()
    m.precompute_embeddings_from_tokens()
    np.testing.assert_allclose(m.entity_embedding_from_tokens.cpu().numpy(), z["E_eval"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(m.relations_embedding_from_tokens.cpu().numpy(), z["R_eval"], rtol=1e-5, atol=2e-6)
    if "sp_all_eval" in z.files:
        out = m.sp_prefix_score(dev(z["sp_subj"]), dev(z["sp_rel"]))
        np.testing.assert_allclose(out.cpu().numpy(), z["sp_all_eval"], rtol=0, atol=1e-4)
    if "po_all_eval" in z.files:
        out = m.po_prefix_score(dev(z["po_rel"]), dev(z["po_obj"]))
        np.testing.assert_allclose(out.cpu().numpy(), z["po_all_eval"], rtol=0, atol=1e-4)


def test_token_pooled_training_trajectory_vs_oracle(okge_lib):
    """three optimisation steps (sum pooling + batch-norm, dropout 0): loss curve and tables against the oracle"""
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep
    z = golden("g9_unigram_sum_bn_shared")
    e, r, _ = slots(z)
    st = TokenPooledTrainStep(e, r, "complex", lr=0.1)
    We, Wr = z["We"].copy(), z["Wr"].copy()
    d = We.shape[1]
    bn_e = dict(weight=z["bn_e_w"].copy(), bias=z["bn_e_b"].copy(), running_mean=np.zeros(d, np.float32), running_var=np.ones(d, np.float32))
    bn_r = dict(weight=z["bn_r_w"].copy(), bias=z["bn_r_b"].copy(), running_mean=np.zeros(d, np.float32), running_var=np.ones(d, np.float32))
    sums = [np.zeros_like(a) for a in (We, Wr, bn_e["weight"], bn_e["bias"], bn_r["weight"], bn_r["bias"])]
    for _ in range(3):
        loss = float(st.step(batch_of(z))[0])
        out = ko.unigram_step_forward_backward(ko.COMPLEX, We, Wr, z["ent_tokens"], z["rel_tokens"], (z["po_rel"], z["po_obj"]),
                                               (z["sp_subj"], z["sp_rel"]), z["cand"], z["labels"], pool="sum", bn_ent=bn_e, bn_rel=bn_r)
        assert abs(loss - out["loss"]) <= 5e-5 * abs(out["loss"])
        params = (We, Wr, bn_e["weight"], bn_e["bias"], bn_r["weight"], bn_r["bias"])
        grads = (out["dWe"], out["dWr"], out["d_bn_ent"][0], out["d_bn_ent"][1], out["d_bn_rel"][0], out["d_bn_rel"][1])
        for p_, g_, s_ in zip(params, grads, sums):
            ko.adagrad_step(p_, g_, s_, 0.1)
    # Adagrad's early steps amplify 1e-12-level gradient differences where |g| is tiny (see adagrad_tol in
    # tests/test_oracle_golden.py); the per-step losses above are the tight check, the tables a coarse one
    st.flush()                              # rows no batch named owe decay-only steps until then (decay_window)
    close = np.isclose(e.W.cpu().numpy(), We, rtol=2e-3, atol=2e-4)
    assert close.mean() > 0.95 and np.abs(e.W.cpu().numpy() - We).max() < 0.3        # at most lr per step
    np.testing.assert_allclose(e.running_mean.cpu().numpy(), bn_e["running_mean"], rtol=0, atol=0.1)     # follows W


@pytest.mark.parametrize("i", range(16))
def test_random_token_pooled_step_vs_oracle(okge_lib, i):
    """random shapes (slot size, token-sequence length incl. the hot-token LDS path and rare tokens, repeated ids,
    one-sided batches) through TokenPooledTrainStep.forward_backward against the oracle"""
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
    rng = np.random.default_rng(4200 + i)
    d = int(rng.choice([8, 24, 64, 100, 256]))
    L = int(rng.choice([1, 3, 10, 17]))
    n_ent, n_rel, vt_e, vt_r = int(rng.integers(30, 400)), int(rng.integers(4, 25)), int(rng.integers(6, 300)), int(rng.integers(6, 60))
    pool = str(rng.choice(["sum", "mean", "max"]))
    bn = bool(rng.random() < 0.6)
    n_po, n_sp = int(rng.integers(0, 70)), int(rng.integers(0, 70))
    if n_po + n_sp == 0:
        n_sp = 7

    def tokens(n, vocab):
        m = np.zeros((n, L), np.int32)
        for r in range(n):
            k = int(rng.integers(1, L + 1))
            m[r, :k] = rng.integers(1, vocab, k)                       # ids < 32 take the LDS path, repeats allowed
        return m
    ent_tok, rel_tok = tokens(n_ent, vt_e), tokens(n_rel, vt_r)
    We = (rng.standard_normal((vt_e, d)) * 0.3).astype(np.float32)
    Wr = (rng.standard_normal((vt_r, d)) * 0.3).astype(np.float32)
    N = int(rng.integers(1, 300))
    cand = rng.integers(2, n_ent, N).astype(np.int32)                   # repeats allowed
    po = (rng.integers(2, n_rel, n_po).astype(np.int32), rng.integers(2, n_ent, n_po).astype(np.int32)) if n_po else None
    sp = (rng.integers(2, n_ent, n_sp).astype(np.int32), rng.integers(2, n_rel, n_sp).astype(np.int32)) if n_sp else None
    B = n_po + n_sp
    y = np.zeros((B, N), np.float32)
    for b in range(B):
        y[b, rng.choice(N, size=int(rng.integers(0, min(3, N) + 1)), replace=False)] = 1
    mk_bn = lambda: dict(weight=rng.random(d).astype(np.float32), bias=(rng.standard_normal(d) * 0.1).astype(np.float32),   # noqa: E731
                         running_mean=np.zeros(d, np.float32), running_var=np.ones(d, np.float32))
    bn_e, bn_r = (mk_bn(), mk_bn()) if bn else (None, None)
    if bn and min(N, n_po or N, n_sp or N) < 2:
        pytest.skip("batch-norm over a single row divides by zero variance in both implementations")
    e = TokenSlot(dev(We), dev(ent_tok), pool, bn, dev(bn_e["weight"]) if bn else None, dev(bn_e["bias"]) if bn else None)
    r = TokenSlot(dev(Wr), dev(rel_tok), pool, bn, dev(bn_r["weight"]) if bn else None, dev(bn_r["bias"]) if bn else None)
    ref = ko.unigram_step_forward_backward(ko.COMPLEX if d % 2 == 0 else ko.DISTMULT, We, Wr, ent_tok, rel_tok, po, sp, cand, y,
                                           pool=pool, bn_ent=bn_e, bn_rel=bn_r)
    st = TokenPooledTrainStep(e, r, "complex" if d % 2 == 0 else "distmult")
    b = PrefixBatch(cand_ids=dev(cand))
    if po:
        b.po_rel, b.po_obj = dev(po[0]), dev(po[1])
    if sp:
        b.sp_subj, b.sp_rel = dev(sp[0]), dev(sp[1])
    b.pos_row, b.pos_col = positives_from_dense(dev(y))
    loss = float(st.forward_backward(b)[0])
    info = dict(i=i, d=d, L=L, pool=pool, bn=bn, n_po=n_po, n_sp=n_sp, N=N)
    assert abs(loss - ref["loss"]) <= 1e-4 * abs(ref["loss"]) + 1e-5, (info, loss, ref["loss"])
    for mine, want in ((e.dW, ref["dWe"]), (r.dW, ref["dWr"])):
        np.testing.assert_allclose(mine.cpu().numpy(), want, rtol=0, atol=2e-4 * np.abs(want).max() + 1e-7, err_msg=str(info))
    if bn:
        np.testing.assert_allclose(e.d_bn[:d].cpu().numpy(), ref["d_bn_ent"][0], rtol=0, atol=2e-4 * np.abs(ref["d_bn_ent"][0]).max() + 1e-7)
        np.testing.assert_allclose(e.running_var.cpu().numpy(), bn_e["running_var"], rtol=1e-4, atol=1e-6)


# ---- round 4: the token-table gradient as store-and-sum through a device-built inverted index (okge_pool.hip "scatter plan") ----
def _plan_case(rng, d, L, n_ent, vt_e, N, n_po, n_sp, pool="sum", bn=False, hot_frac=0.3, mid_tokens=()):
    """token matrices with a chosen mix: ids < 32 (LDS slabs), a few mid-frequency ids >= 32 that land in MANY rows
    (segments longer than one wave sorts: the bitmap path), rare ids (wave-sorted segments), repeats inside a row"""
    def tokens(n, vocab):
        m = np.zeros((n, L), np.int32)
        for r in range(n):
            k = int(rng.integers(1, L + 1))
            row = rng.integers(32, vocab, k)
            hot = rng.random(k) < hot_frac
            row[hot] = rng.integers(1, 32, int(hot.sum()))
            for t in mid_tokens:
                if rng.random() < 0.5:
                    row[int(rng.integers(0, k))] = t
            if k > 1 and rng.random() < 0.3:
                row[1] = row[0]                                   # the same token twice in one row: two pairs
            m[r, :k] = row
        return m
    n_rel, vt_r = 40, 50
    ent_tok = tokens(n_ent, vt_e)
    mid_tokens = (45,) if mid_tokens else ()                  # (the relation vocabulary is smaller)
    rel_tok = tokens(n_rel, vt_r)
    We = (rng.standard_normal((vt_e, d)) * 0.3).astype(np.float32)
    Wr = (rng.standard_normal((vt_r, d)) * 0.3).astype(np.float32)
    cand = rng.integers(2, n_ent, N).astype(np.int32)
    po = (rng.integers(2, n_rel, n_po).astype(np.int32), rng.integers(2, n_ent, n_po).astype(np.int32))
    sp = (rng.integers(2, n_ent, n_sp).astype(np.int32), rng.integers(2, n_rel, n_sp).astype(np.int32))
    B = n_po + n_sp
    y = np.zeros((B, N), np.float32)
    y[np.arange(B), rng.integers(0, N, B)] = 1
    mk_bn = lambda: dict(weight=rng.random(d).astype(np.float32), bias=(rng.standard_normal(d) * 0.1).astype(np.float32),   # noqa: E731
                         running_mean=np.zeros(d, np.float32), running_var=np.ones(d, np.float32))
    return dict(We=We, Wr=Wr, ent_tok=ent_tok, rel_tok=rel_tok, cand=cand, po=po, sp=sp, y=y, pool=pool,
                bn_e=mk_bn() if bn else None, bn_r=mk_bn() if bn else None)


def _plan_step(c, scorer="complex", **kw):
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
    bn = c["bn_e"] is not None
    e = TokenSlot(dev(c["We"]), dev(c["ent_tok"]), c["pool"], bn, dev(c["bn_e"]["weight"]) if bn else None, dev(c["bn_e"]["bias"]) if bn else None)
    r = TokenSlot(dev(c["Wr"]), dev(c["rel_tok"]), c["pool"], bn, dev(c["bn_r"]["weight"]) if bn else None, dev(c["bn_r"]["bias"]) if bn else None)
    st = TokenPooledTrainStep(e, r, scorer, **kw)
    b = PrefixBatch(cand_ids=dev(c["cand"]), po_rel=dev(c["po"][0]), po_obj=dev(c["po"][1]), sp_subj=dev(c["sp"][0]), sp_rel=dev(c["sp"][1]))
    b.pos_row, b.pos_col = positives_from_dense(dev(c["y"]))
    return st, e, r, b


@pytest.mark.parametrize("case", ["short", "long_one_window", "long_two_windows", "mean_bn", "d256_bn"])
def test_scatter_plan_matches_oracle_and_is_bit_reproducible(okge_lib, case):
    """the same step three times from cleared gradients: token-table gradients EQUAL bit for bit (the atomics' sums moved in
    the last bits), within tolerance of the float64 oracle and of the atomics path; every segment class is met"""
    rng = np.random.default_rng({"short": 1, "long_one_window": 2, "long_two_windows": 3, "mean_bn": 4, "d256_bn": 5}[case])
    if case == "short":
        c = _plan_case(rng, d=8, L=5, n_ent=300, vt_e=4000, N=200, n_po=30, n_sp=20)
    elif case == "long_one_window":
        c = _plan_case(rng, d=24, L=6, n_ent=900, vt_e=600, N=1500, n_po=100, n_sp=90, mid_tokens=(40, 77, 311))
    elif case == "long_two_windows":                           # (N + B) * L = 8 200 * 17 > 131 072 pair indices
        c = _plan_case(rng, d=8, L=17, n_ent=5000, vt_e=3000, N=7000, n_po=700, n_sp=500, mid_tokens=(33, 1500))
    elif case == "mean_bn":
        c = _plan_case(rng, d=64, L=4, n_ent=500, vt_e=200, N=700, n_po=64, n_sp=64, pool="mean", bn=True, mid_tokens=(50,))
    else:
        c = _plan_case(rng, d=256, L=10, n_ent=800, vt_e=900, N=600, n_po=70, n_sp=70, bn=True, mid_tokens=(64,))
    kind = ko.COMPLEX
    ref = ko.unigram_step_forward_backward(kind, c["We"], c["Wr"], c["ent_tok"], c["rel_tok"], c["po"], c["sp"], c["cand"], c["y"],
                                           pool=c["pool"], bn_ent=c["bn_e"], bn_rel=c["bn_r"])
    st, e, r, b = _plan_step(c)
    runs = []
    for _ in range(3):
        e.dW.zero_(); r.dW.zero_()
        st.forward_backward(b)
        torch.cuda.synchronize()
        runs.append((e.dW.clone(), r.dW.clone()))
    for dWe, dWr in runs[1:]:
        assert torch.equal(dWe, runs[0][0]) and torch.equal(dWr, runs[0][1])
    for mine, want in ((runs[0][0], ref["dWe"]), (runs[0][1], ref["dWr"])):
        np.testing.assert_allclose(mine.cpu().numpy(), want, rtol=0, atol=2e-4 * np.abs(want).max() + 1e-7)
    # every stamped row and only those: rows with a gradient carry the stamp
    for sl, dW in ((e, runs[0][0]), (r, runs[0][1])):
        nz = (dW != 0).any(dim=1)
        stamped = sl.touched == sl.stamp
        assert bool((stamped | ~nz).all()), "a row with a gradient is not stamped"
    # the atomics path on the same inputs
    st2, e2, r2, b2 = _plan_step(c)
    st2.pool.scatter = "atomics"
    st2.forward_backward(b2)
    torch.cuda.synchronize()
    for a, o in ((e2.dW, runs[0][0]), (r2.dW, runs[0][1])):
        np.testing.assert_allclose(a.cpu().numpy(), o.cpu().numpy(), rtol=0, atol=1e-5 * float(o.abs().max()) + 1e-9)
    from open_knowledge_graph_embeddings_amd import _native as N
    N.check_ids()


def test_touched_map_adagrad_is_bit_equal_to_the_dense_sweep(okge_lib):
    """three optimisation steps with the touched-row map (gradient rows no token named are neither read nor cleared) against
    the same steps with the map switched off: tables and accumulators bit-equal"""
    rng = np.random.default_rng(11)
    c = _plan_case(rng, d=64, L=5, n_ent=400, vt_e=3000, N=300, n_po=40, n_sp=40, bn=True, mid_tokens=(45,))
    a = _plan_step(c, decay_window=1)
    b_ = _plan_step(c, decay_window=1)
    b_[1].touched = b_[2].touched = None                         # dense sweep: every gradient row is read
    for _ in range(3):
        a[0].step(a[3])
        b_[0].step(b_[3])
    torch.cuda.synchronize()
    for x, y in ((a[1], b_[1]), (a[2], b_[2])):
        assert torch.equal(x.W, y.W) and torch.equal(x.sumW, y.sumW) and torch.equal(x.bn, y.bn)
        assert float(x.dW.abs().max()) == 0.0                    # cleared where stamped, zero elsewhere


def _lazy_problem(seed=31):
    rng = np.random.default_rng(seed)
    return _plan_case(rng, d=64, L=6, n_ent=2000, vt_e=5000, N=900, n_po=96, n_sp=96, bn=True, mid_tokens=(45,))


def _lazy_make(c, window, **kw):
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
    e = TokenSlot(dev(c["We"]), dev(c["ent_tok"]), "sum", True, dev(c["bn_e"]["weight"]), dev(c["bn_e"]["bias"]))
    r = TokenSlot(dev(c["Wr"]), dev(c["rel_tok"]), "sum", True, dev(c["bn_r"]["weight"]), dev(c["bn_r"]["bias"]))
    return TokenPooledTrainStep(e, r, "complex", lr=0.1, dropout=0.1, seed=3, decay_window=window, **kw), e, r


def _lazy_batch(r2, n_ent=2000, n_rel=40, N=900, B=192, lo=2):
    """a batch over entity ids [lo, n_ent): different token rows named step after step"""
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    y = np.zeros((B, N), np.float32)
    y[np.arange(B), r2.integers(0, N, B)] = 1
    b = PrefixBatch(cand_ids=dev(r2.integers(lo, n_ent, N).astype(np.int32)),
                    po_rel=dev(r2.integers(2, n_rel, B // 2).astype(np.int32)), po_obj=dev(r2.integers(lo, n_ent, B // 2).astype(np.int32)),
                    sp_subj=dev(r2.integers(lo, n_ent, B // 2).astype(np.int32)), sp_rel=dev(r2.integers(2, n_rel, B // 2).astype(np.int32)))
    b.pos_row, b.pos_col = positives_from_dense(dev(y))
    return b


def _same_tables(a, b_):
    for x, y_ in ((a[1], b_[1]), (a[2], b_[2])):
        assert torch.equal(x.W, y_.W) and torch.equal(x.sumW, y_.sumW), "token table / accumulator differ"
        assert torch.equal(x.bn, y_.bn) and torch.equal(x.sum_bn, y_.sum_bn)
        assert float(x.dW.abs().max()) == 0.0 and float(y_.dW.abs().max()) == 0.0


@pytest.mark.parametrize("window", [2, 3, 8, 64])
def test_lazy_decay_is_bit_equal_to_the_eager_sweep(okge_lib, window):
    """decay_window > 1 (okge_adagrad_lazy + okge_pool_catch_up_calls: the weight-decay-only Adagrad steps of token rows no
    batch names are deferred and replayed in registers) against decay_window = 1 (every row every step, the reference's
    order): every step's loss bit-equal (the forward reads caught-up rows), tables / accumulators / batch-norm parameters
    bit-equal after flush() -- over 14 steps of DIFFERENT batches whose ids move through the table (rows go cold and come
    back), with a flush in the middle and a learning-rate change while steps are pending"""
    c = _lazy_problem()
    a, b_ = _lazy_make(c, window), _lazy_make(c, 1)
    assert a[0].decay_window == window and b_[0].decay_window == 1
    r2 = np.random.default_rng(5)
    for step in range(14):
        lo = 2 + (step % 5) * 290                                  # ids [lo, lo + 800): a sliding part of the entities
        st0 = r2.bit_generator.state
        losses = []
        for st, _, _ in (a, b_):
            r2.bit_generator.state = st0
            losses.append(float(st.step(_lazy_batch(r2, n_ent=lo + 800, lo=lo))[0]))
        assert losses[0] == losses[1], (step, losses)
        if step == 6:
            a[0].flush()
            torch.cuda.synchronize()
            _same_tables(a, b_)
            assert int(a[1].row_steps.min()) == int(a[1].row_steps.max()) == 7 == int(a[0]._counters[0])
        if step == 9:
            a[0].lr = b_[0].lr = 0.05                              # pending steps keep the rate of their time
    lag = int(a[0]._counters[0]) - a[1].row_steps
    assert int(lag.max()) <= window and int(lag.min()) >= 0
    if window <= 8:
        assert int(lag.max()) > 0, "nothing was deferred: the test does not exercise the replay"
    a[0].flush()
    torch.cuda.synchronize()
    _same_tables(a, b_)
    assert int(a[1].touched.max()) == 0 and int(a[2].touched.max()) == 0          # the map is clean after every update
    from open_knowledge_graph_embeddings_amd import _native as N
    N.check_ids()


def test_lazy_decay_with_warm_accumulators_and_state_snapshot(okge_lib):
    """accumulators that have seen real gradients: the decay term is below half an ulp, a replayed step returns its input
    bits and the replay loop ends early -- still bit-equal; state_tensors() flushes and carries the step counters, so a
    snapshot / restore (GraphedTrainStep's warm-up) is exact"""
    c = _lazy_problem(32)
    a, b_ = _lazy_make(c, 8), _lazy_make(c, 1)
    for st, e, r in (a, b_):
        e.sumW.fill_(1e-4)
        r.sumW.fill_(1e-4)
    r2 = np.random.default_rng(6)
    snap = None
    for step in range(10):
        st0 = r2.bit_generator.state
        for st, _, _ in (a, b_):
            r2.bit_generator.state = st0
            st.step(_lazy_batch(r2))
        if step == 4:
            snap = [t.clone() for t in a[0].state_tensors()]
    a[0].flush()
    torch.cuda.synchronize()
    _same_tables(a, b_)
    final = [t.clone() for t in a[0].state_tensors()]
    for t, s0 in zip(a[0].state_tensors(), snap):                  # back to step 5, the same five batches again
        t.copy_(s0)
    a[0].steps = 5
    r2 = np.random.default_rng(6)
    for step in range(10):
        b = _lazy_batch(r2)
        if step >= 5:
            a[0].step(b)
    for t, f in zip(a[0].state_tensors(), final):
        assert torch.equal(t, f)


def test_lazy_decay_under_graph_replay(okge_lib):
    """the step with deferred decay captured in a HIP graph (device-side step counter, catch-up and lazy update inside the
    graph): tables bit-equal to the eager sweep launched step by step"""
    from open_knowledge_graph_embeddings_amd.train_step import GraphedTrainStep
    c = _lazy_problem(33)
    a, b_ = _lazy_make(c, 4), _lazy_make(c, 1)
    r2 = np.random.default_rng(7)
    batches = [_lazy_batch(r2, n_ent=600 + 400 * i, lo=2 + 300 * i) for i in range(4)]
    cap = max(b.nnz for b in batches)
    g = GraphedTrainStep(a[0], batches[0], pos_capacity=cap)
    for i in range(9):
        la = float(g.step(batches[i % 4])[0])
        lb = float(b_[0].step(batches[i % 4])[0])
        assert la == lb, (i, la, lb)
        if i == 4:                                                 # a reader in the middle of the run: flush, then go on replaying
            a[0].flush()
            torch.cuda.synchronize()
            _same_tables(a, b_)
    a[0].flush()
    torch.cuda.synchronize()
    _same_tables(a, b_)


def test_module_readers_flush_the_training_driver(okge_lib):
    """UnigramPooling*RelationModel.train_step() updates the module's parameters in place with deferred decay: the module's
    own readers (eval-mode precompute, state_dict) see the tables of the eager sweep"""
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.token_pooled import UnigramPoolingComplexRelationModel
    rng = np.random.default_rng(9)
    n_ent, n_rel, vt, L, d = 300, 20, 900, 4, 32
    md = EntityRelationDatasetMeta(entities_size=n_ent, relations_size=n_rel, entity_tokens_size=vt, relation_tokens_size=60, max_length=(L, L),
                                   entity_id_to_tokens_map=[[int(t) for t in rng.integers(1, vt, L)] for _ in range(n_ent)],
                                   relation_id_to_tokens_map=[[int(t) for t in rng.integers(1, 60, L)] for _ in range(n_rel)])
    outs = []
    for window in (8, 1):
        torch.manual_seed(0)
        m = UnigramPoolingComplexRelationModel(entity_slot_size=d, relation_slot_size=d, train_data=md, pool="sum", normalize="batchnorm",
                                               dropout=0.0, init_std=0.3).cuda()
        st = m.train_step(lr=0.1)
        st.decay_window = window                # (tables this small default to 1)
        r2 = np.random.default_rng(4)
        for _ in range(5):
            st.step(_lazy_batch(r2, n_ent=n_ent, n_rel=n_rel, N=64, B=32))
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        m.eval()
        with torch.no_grad():
            m.precompute_embeddings_from_tokens()
        outs.append((sd, m.entity_embedding_from_tokens.clone()))
    for k in outs[0][0]:
        assert torch.equal(outs[0][0][k], outs[1][0][k]), k
    assert torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("window", [1, 5])
def test_fast_decay_arithmetic_is_the_generic_one(okge_lib, window):
    """the replay of deferred decay steps runs packed, branch-free copies of the compiler's correctly rounded sqrt / division
    where every operand of a row is an ordinary number (okge_adagrad_device.h, decay_step4_ordinary) and the generic code elsewhere:
    against the eager sweep (okge_adagrad_multi: generic code throughout) the tables must be bit-equal -- rows of ordinary
    numbers over twelve orders of magnitude (fast path), rows with zeros, denormal-range accumulators, tiny and huge
    parameters (generic path), several steps deep"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    eng = H.HotPath(torch.device("cuda:0"))
    g = torch.Generator(device="cuda").manual_seed(17)
    rows, d = 6144, 256
    u = lambda lo, hi: 10.0 ** (lo + (hi - lo) * torch.rand((rows, d), device="cuda", generator=g))      # noqa: E731
    sign = torch.where(torch.rand((rows, d), device="cuda", generator=g) < 0.5, -1.0, 1.0)
    p = sign * u(-12, 4)
    s = u(-27, 10)
    p[:2048] = (sign * u(-6, 1))[:2048]                      # ordinary rows: every element inside the fast path's range
    s[:2048] = u(-26, 8)[:2048]
    s[2048:3072] = 0.0                                        # first steps of a run
    p[3072:3200, ::7] = 0.0
    s[3200:3328] = u(-44, -30)[3200:3328]                     # accumulators below 2^-96: the scaled sqrt
    p[3328:3456] = (sign * u(-30, -14))[3328:3456]
    p[3456:3584] = (sign * u(5, 12))[3456:3584]
    for lr, wd, eps in ((0.1, 1e-10, 1e-8), (0.3, 1e-6, 1e-8), (0.05, 1e-10, 1e-10), (0.1, 0.5, 1e-8)):      # (the last: parameters outside)
        pe, se, ge = p.clone(), s.clone(), torch.zeros_like(p)
        pl, sl, gl = p.clone(), s.clone(), torch.zeros_like(p)
        steps_ = torch.zeros(rows, dtype=torch.int32, device="cuda")
        maps = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        lazy = [(pl, gl, sl, steps_, maps, 1)]
        for step in range(7):
            # a third of the rows carry a gradient (stamped in the lazy run: what they owe, then the step with the gradient):
            # ordinary magnitudes in the first rows, twenty orders of magnitude and zeros elsewhere
            sel = torch.rand(rows, device="cuda", generator=g) < 0.33
            grad = sign * u(-14, 3)
            grad[:2048] = (sign * u(-7, -1))[:2048]
            grad[:, step::11] = 0.0
            for gbuf in (ge, gl):
                gbuf[sel] = grad[sel]
            maps[sel] = 1
            eng.adagrad_multi([(pe, ge, se)], lr, wd, eps)
            eng.adagrad_lazy(lazy, cnt, window, False, lr, wd, eps)
            assert int(maps.max()) == 0 and float(gl.abs().max()) == 0.0 and float(ge.abs().max()) == 0.0
        eng.adagrad_lazy(lazy, cnt, window, True, lr, wd, eps)
        torch.cuda.synchronize()
        assert int(cnt[0]) == 7 and int(steps_.min()) == 7
        same_p, same_s = (pe.view(torch.int32) == pl.view(torch.int32)), (se.view(torch.int32) == sl.view(torch.int32))
        assert bool(same_p.all()) and bool(same_s.all()), (lr, wd, eps, int((~same_p).sum()), int((~same_s).sum()),
                                                           (~(same_p & same_s)).any(dim=1).nonzero()[:8].flatten().tolist())
        assert not torch.equal(pe, p)                         # (the steps did move the table)


@pytest.mark.parametrize("window", [1, 3, 8])
def test_twelve_reference_optimizer_steps_with_rows_no_batch_names(okge_lib, window):
    """G16: the reference's UnigramPoolingComplexRelationModel through twelve steps of ITS OWN OptimRegime Adagrad (weight_decay
    1e-10, the leaked eps 1e-8) on batches that move through the entity ids.  107 of the 300 entity token rows are named by no
    entity at all -- the reference's dense optimizer still moves them, every step, by their weight-decay term alone (up to 0.013
    over the run): the premise of okge_adagrad_lazy.  This build, with every window: the first loss within 5e-5, the never-named
    rows and their accumulators within a few ulps per step of the reference's (same IEEE operations; torch rounds g*g and
    lr*(g/std) separately where the kernels use fused multiply-adds); the named rows only coarsely (see the loop)."""
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
    z = golden("g16_unigram_adagrad")
    e = TokenSlot(dev(z["We"]), dev(z["ent_tokens"]), "sum", True, dev(z["bn_e_w"]), dev(z["bn_e_b"]))
    r = TokenSlot(dev(z["Wr"]), dev(z["rel_tokens"]), "sum", True, dev(z["bn_r_w"]), dev(z["bn_r_b"]))
    st = TokenPooledTrainStep(e, r, "complex", lr=float(z["opt_lr"]), weight_decay=float(z["opt_weight_decay"]), eps=float(z["opt_eps"]),
                              decay_window=window)
    assert st.decay_window == window and float(z["opt_eps"]) == 1e-8
    for s in range(int(z["nsteps"])):
        b = PrefixBatch(po_rel=dev(z[f"s{s}_po_rel"].reshape(-1)), po_obj=dev(z[f"s{s}_po_obj"].reshape(-1)),
                        sp_subj=dev(z[f"s{s}_sp_subj"].reshape(-1)), sp_rel=dev(z[f"s{s}_sp_rel"].reshape(-1)),
                        cand_ids=dev(z[f"s{s}_cand"].reshape(-1).astype(np.int32)))
        b.pos_row, b.pos_col = positives_from_dense(dev(z[f"s{s}_labels"]))
        loss = float(st.step(b)[0])
        # the first step is the reference's to 5e-5; from the second on the runs are different samples of an ill-conditioned
        # trajectory -- Adagrad's first steps turn gradient entries of rounding-noise size (batch-norm makes the gradient of a
        # token that stands in every row cancel to ~1e-9) into +-lr * g / (|g| + 1e-8) ~ 0.01 moves.  The oracle's own curve
        # leaves the reference's by up to 0.9 % in float64 and 1.7 % in float32 over these twelve steps (same algorithm, other
        # rounding); this build by about 2 %
        assert abs(loss - float(z[f"s{s}_loss"])) <= (5e-5 if s == 0 else 6e-2) * abs(float(z[f"s{s}_loss"])), (s, loss, float(z[f"s{s}_loss"]))
    st.flush()
    torch.cuda.synchronize()
    named = np.zeros(z["We"].shape[0], bool)
    named[np.unique(z["ent_tokens"])] = True
    W, S = e.W.cpu().numpy(), e.sumW.cpu().numpy()
    assert (~named).sum() == 107 and np.abs(z["We_end"][~named] - z["We"][~named]).max() > 0.01     # the reference moved them
    np.testing.assert_allclose(W[~named], z["We_end"][~named], rtol=2e-5, atol=1e-9)
    np.testing.assert_allclose(S[~named], z["sumWe_end"][~named], rtol=2e-5, atol=1e-30)
    diff = np.abs(W[named] - z["We_end"][named])
    print("named rows: share within 1e-3:", float((diff < 1e-3).mean()), "max:", float(diff.max()))
    assert (diff < 0.05).mean() > 0.9 and diff.max() < 12 * float(z["opt_lr"])         # coarse: see above


@pytest.mark.parametrize("pool", ["max", "sum_atomics"])
def test_lazy_decay_on_the_atomics_backward(okge_lib, pool):
    """the deferred decay behind the float-atomic token-table scatter (max pooling always takes it; the pool engine's scatter = "atomics"
    for the others): the backward's sums differ in the last bits from run to run there, so the rows a batch names are compared to a
    tolerance -- but every row NO batch named must still equal the eager run bit for bit after flush(), and the map must be clean"""
    rng = np.random.default_rng(41)
    c = _plan_case(rng, d=64, L=5, n_ent=900, vt_e=6000, N=300, n_po=48, n_sp=48, pool="max" if pool == "max" else "sum", bn=True)
    a, b_ = _plan_step(c, decay_window=4), _plan_step(c, decay_window=1)
    if pool == "sum_atomics":
        a[0].pool.scatter = b_[0].pool.scatter = "atomics"
    assert a[0].decay_window == 4 and not a[0].pool.scatter_plan([(a[1],)])
    for _ in range(7):
        a[0].step(a[3])
        b_[0].step(b_[3])
    a[0].flush()
    torch.cuda.synchronize()
    named = torch.zeros(c["We"].shape[0], dtype=torch.bool, device="cuda")
    ids = torch.cat([dev(c["cand"]), dev(c["po"][1]), dev(c["sp"][0])]).long()
    named[dev(c["ent_tok"])[ids].reshape(-1).long()] = True
    assert int((~named).sum()) > 1000
    assert torch.equal(a[1].W[~named], b_[1].W[~named]) and torch.equal(a[1].sumW[~named], b_[1].sumW[~named])
    np.testing.assert_allclose(a[1].W[named].cpu().numpy(), b_[1].W[named].cpu().numpy(), rtol=1e-3, atol=1e-4)
    assert int(a[1].touched.max()) == 0 and float(a[1].dW.abs().max()) == 0.0


@pytest.mark.parametrize("d", [8, 200, 512])
def test_lazy_decay_other_slot_sizes(okge_lib, d):
    """the deferred decay at slot sizes other than 64 / 256: rows of 2 and 50 column quads (part of a wave idle) and of 128 (two
    trips per row: the column loop of lazy_rows) -- bit-equal to the eager sweep after seven steps of moving batches"""
    from open_knowledge_graph_embeddings_amd.token_pooled import TokenPooledTrainStep, TokenSlot
    rng = np.random.default_rng(50 + d)
    c = _plan_case(rng, d=d, L=5, n_ent=1500, vt_e=4000, N=256, n_po=32, n_sp=32, bn=True)

    def make(window):
        e = TokenSlot(dev(c["We"]), dev(c["ent_tok"]), "sum", True, dev(c["bn_e"]["weight"]), dev(c["bn_e"]["bias"]))
        r = TokenSlot(dev(c["Wr"]), dev(c["rel_tok"]), "sum", True, dev(c["bn_r"]["weight"]), dev(c["bn_r"]["bias"]))
        return TokenPooledTrainStep(e, r, "complex", lr=0.1, dropout=0.0, seed=3, decay_window=window), e, r
    a, b_ = make(3), make(1)
    r2 = np.random.default_rng(8)
    for step in range(7):
        lo = 2 + (step % 3) * 400
        st0 = r2.bit_generator.state
        losses = []
        for st, _, _ in (a, b_):
            r2.bit_generator.state = st0
            losses.append(float(st.step(_lazy_batch(r2, n_ent=lo + 600, N=256, B=64, lo=lo))[0]))
        assert losses[0] == losses[1], (step, losses)
    assert int((int(a[0]._counters[0]) - a[1].row_steps).max()) > 0
    a[0].flush()
    torch.cuda.synchronize()
    _same_tables(a, b_)


def test_model_train_step_masks_relation_rows_with_relation_dropout(okge_lib):
    """UnigramPooling*RelationModel.train_step() hands the step BOTH probabilities (model.py:755-758, :794-795).  Entity
    dropout 0, relation dropout 0.5, lr 0 (the parameters stay put): the relation rows' masks change with the step count, so two
    steps on the same batch give different losses; with relation_dropout=None (it falls back to the entity probability, 0) no
    row is masked and the two losses are bit-equal."""
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.hotpath import PrefixBatch, positives_from_dense
    from open_knowledge_graph_embeddings_amd.token_pooled import UnigramPoolingComplexRelationModel
    rng = np.random.default_rng(21)
    n_ent, n_rel, vt_e, vt_r, d, B = 40, 7, 30, 12, 8, 6
    md = EntityRelationDatasetMeta(entities_size=n_ent, relations_size=n_rel, entity_tokens_size=vt_e, relation_tokens_size=vt_r, max_length=(4, 3),
                                   entity_id_to_tokens_map=[[int(t) for t in rng.integers(1, vt_e, 4)] for _ in range(n_ent)],
                                   relation_id_to_tokens_map=[[int(t) for t in rng.integers(1, vt_r, 3)] for _ in range(n_rel)])
    y = np.zeros((B, n_ent - 2), np.float32)
    y[np.arange(B), rng.integers(0, n_ent - 2, B)] = 1
    batch = PrefixBatch(po_rel=dev(rng.integers(2, n_rel, B // 2).astype(np.int32)), po_obj=dev(rng.integers(2, n_ent, B // 2).astype(np.int32)),
                        sp_subj=dev(rng.integers(2, n_ent, B // 2).astype(np.int32)), sp_rel=dev(rng.integers(2, n_rel, B // 2).astype(np.int32)),
                        cand_first=2, n_cand=n_ent - 2)                                    # 1-vs-all
    batch.pos_row, batch.pos_col = positives_from_dense(dev(y))
    losses = {}
    for relation_dropout in (0.5, None):
        torch.manual_seed(3)
        m = UnigramPoolingComplexRelationModel(entity_slot_size=d, relation_slot_size=d, train_data=md, pool="sum", normalize=None, dropout=0.0,
                                               relation_dropout=relation_dropout, init_std=0.3).cuda()
        st = m.train_step(lr=0.0)
        losses[relation_dropout] = [float(st.step(batch)[0]) for _ in range(2)]
        print("relation_dropout", relation_dropout, "losses", losses[relation_dropout])
    assert losses[0.5][0] != losses[0.5][1]
    assert losses[None][0] == losses[None][1]
