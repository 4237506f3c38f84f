"""Randomised shape sweep of the fused step against the oracle (GPU): slot sizes across every kernel width incl. odd
ones, one-sided batches, tiny and ragged candidate lists with repeats, both losses, label smoothing, Philox dropout on
every stream, forced batch splits, zeroed-gradient fast path.  Seeds are fixed: failures reproduce."""
import numpy as np
import pytest
import torch

from oracle import kge_oracle as ko
from test_hip_parity import dev, make_batch, oracle_step

pytestmark = pytest.mark.gpu


def case(i):
    rng = np.random.default_rng(7000 + i)
    scorer = "complex" if rng.random() < 0.6 else "distmult"
    d = int(rng.choice([2, 6, 16, 30, 64, 100, 130, 200, 208, 256, 300, 400, 512]))
    if scorer == "distmult" and rng.random() < 0.5:
        d = int(rng.choice([1, 3, 17, 63, 129, 257]))                     # odd slot sizes (scalar paths)
    n_ent = int(rng.integers(40, 900))
    n_rel = int(rng.integers(4, 30))
    n_po, n_sp = int(rng.integers(0, 90)), int(rng.integers(0, 90))
    if n_po + n_sp == 0:
        n_po = 5
    mode = rng.choice(["all", "subset", "repeats", "one"])
    if mode == "all":
        cand = np.arange(2, n_ent)
    elif mode == "subset":
        cand = rng.permutation(np.arange(2, n_ent))[: int(rng.integers(1, n_ent - 2))]
    elif mode == "repeats":
        cand = rng.integers(2, n_ent, int(rng.integers(2, 400)))
    else:
        cand = rng.integers(2, n_ent, 1)
    loss = "kl" if rng.random() < 0.3 else "bce"
    smoothing = float(rng.choice([0.0, 0.0, 0.1])) if loss == "bce" else 0.0
    p = float(rng.choice([0.0, 0.0, 0.3, 0.5]))
    p_rel = float(rng.choice([0.0, 0.2])) if p > 0 else 0.0
    split = str(int(rng.choice([0, 0, 1, 2, 5])))
    return dict(i=i, scorer=scorer, d=d, n_ent=n_ent, n_rel=n_rel, n_po=n_po, n_sp=n_sp, cand=cand.astype(np.int32), loss=loss,
                smoothing=smoothing, p=p, p_rel=p_rel, split=split, grads_zero=bool(rng.random() < 0.5), rng=rng)


@pytest.mark.parametrize("i", range(48))
def test_random_shape(okge_lib, monkeypatch, i):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    c = case(i)
    rng, d, B, Nc = c["rng"], c["d"], c["n_po"] + c["n_sp"], len(c["cand"])
    E = (rng.standard_normal((c["n_ent"], d)) * 0.4).astype(np.float32)
    R = (rng.standard_normal((c["n_rel"], d)) * 0.4).astype(np.float32)
    z = {}
    if c["n_po"]:
        z["po_rel"], z["po_obj"] = rng.integers(2, c["n_rel"], c["n_po"]).astype(np.int32), rng.integers(2, c["n_ent"], c["n_po"]).astype(np.int32)
    if c["n_sp"]:
        z["sp_subj"], z["sp_rel"] = rng.integers(2, c["n_ent"], c["n_sp"]).astype(np.int32), rng.integers(2, c["n_rel"], c["n_sp"]).astype(np.int32)
    y = np.zeros((B, Nc), np.float32)
    for b in range(B):
        y[b, rng.choice(Nc, size=int(rng.integers(0, min(4, Nc) + 1)), replace=False)] = 1        # rows without labels too
    seed, step = 0xABCDEF12345 + i, 3 + i
    kw = {}
    if c["p"] > 0:
        kw = dict(p_ent=c["p"], p_rel=c["p_rel"],
                  keep_cand=ko.dropout_keep_mask(seed, H.STREAM_CAND, step, Nc, d, c["p"]),
                  keep_po_ent=ko.dropout_keep_mask(seed, H.STREAM_PO_ENT, step, c["n_po"], d, c["p"]) if c["n_po"] else None,
                  keep_sp_ent=ko.dropout_keep_mask(seed, H.STREAM_SP_ENT, step, c["n_sp"], d, c["p"]) if c["n_sp"] else None)
        if c["p_rel"] > 0:
            kw.update(keep_po_rel=ko.dropout_keep_mask(seed, H.STREAM_PO_REL, step, c["n_po"], d, c["p_rel"]) if c["n_po"] else None,
                      keep_sp_rel=ko.dropout_keep_mask(seed, H.STREAM_SP_REL, step, c["n_sp"], d, c["p_rel"]) if c["n_sp"] else None)
    ref = oracle_step(c["scorer"], E, R, z, c["cand"], y, c["loss"], c["smoothing"], **kw)
    batch = make_batch(z, c["cand"], c["n_ent"], labels=y)
    if c["p"] > 0:
        batch.drop_cand = H.DropoutSpec(c["p"], seed, H.STREAM_CAND, step)
        batch.drop_po_ent = H.DropoutSpec(c["p"], seed, H.STREAM_PO_ENT, step)
        batch.drop_sp_ent = H.DropoutSpec(c["p"], seed, H.STREAM_SP_ENT, step)
        batch.drop_po_rel = H.DropoutSpec(c["p_rel"], seed, H.STREAM_PO_REL, step)
        batch.drop_sp_rel = H.DropoutSpec(c["p_rel"], seed, H.STREAM_SP_REL, step)
    if c["split"] != "0":
        monkeypatch.setenv("OKGE_B_SPLIT", c["split"])
    hp = H.HotPath("cuda:0")
    Et, Rt = dev(E), dev(R)
    dE, dR = torch.zeros_like(Et), torch.zeros_like(Rt)
    scores = torch.empty((B, (Nc + 3) // 4 * 4), device="cuda:0")[:, :Nc]
    loss = hp.forward_backward(Et, Rt, c["scorer"], batch, dE, dR, loss=c["loss"], label_smoothing=c["smoothing"],
                               scores=scores, grads_zero=c["grads_zero"])
    torch.cuda.synchronize()
    info = {k: v for k, v in c.items() if k not in ("rng", "cand")}
    np.testing.assert_allclose(scores.cpu().numpy(), ref["outputs"], rtol=0, atol=1e-4, err_msg=str(info))
    # + an absolute term: a single-candidate KL loss is exactly 0 in the oracle and ~1e-6 of exp/log rounding here
    assert abs(loss.item() - ref["loss"]) <= 5e-5 * abs(ref["loss"]) + 1e-5, (info, loss.item(), ref["loss"])
    for mine, r in ((dE, ref["dE"]), (dR, ref["dR"])):
        np.testing.assert_allclose(mine.cpu().numpy(), r, rtol=0, atol=5e-5 * np.abs(r).max() + 5e-7, err_msg=str(info))   # + exp/log noise where the true gradient is 0 (600 further seeds pass)


@pytest.mark.parametrize("i", range(8))
def test_random_shape_more_tiles_than_cus(okge_lib, monkeypatch, i):
    """the same sweep where the candidate tiles outnumber the CUs (N 16.5 k .. 40 k, B 192 .. 700): rounds of one workgroup
    per CU, the leftover tiles launched apart with the rows split across workgroups (okge_plan.h tail_split), candidate
    ranges of whole rounds when the G^T budget is forced small -- against the oracle, both losses, dropout, id lists"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(8100 + i)
    scorer = "complex" if i % 2 == 0 else "distmult"
    d = int(rng.choice([8, 64, 130, 200, 256]))
    N = int(rng.integers(16500, 40000))
    n_ent, n_rel = N + 2 + int(rng.integers(0, 300)), int(rng.integers(5, 40))
    n_po, n_sp = int(rng.integers(90, 360)), int(rng.integers(100, 340))
    B = n_po + n_sp
    cand = np.arange(2, 2 + N) if i % 3 else (2 + rng.permutation(n_ent - 2)[:N])
    loss = "kl" if i % 4 == 1 else "bce"
    smoothing = 0.1 if i % 4 == 2 else 0.0
    p = float(rng.choice([0.0, 0.3]))
    E = (rng.standard_normal((n_ent, d)) * 0.4).astype(np.float32)
    R = (rng.standard_normal((n_rel, d)) * 0.4).astype(np.float32)
    z = dict(po_rel=rng.integers(2, n_rel, n_po).astype(np.int32), po_obj=rng.integers(2, n_ent, n_po).astype(np.int32),
             sp_subj=rng.integers(2, n_ent, n_sp).astype(np.int32), sp_rel=rng.integers(2, n_rel, n_sp).astype(np.int32))
    y = np.zeros((B, N), np.float32)
    for b in range(B):
        y[b, rng.choice(N, size=int(rng.integers(0, 4)), replace=False)] = 1
    y[0, N - 1] = y[B - 1, N - 1] = y[B // 2, 64 * (N // 64 // 256 * 256)] = 1           # positives inside the tail tiles
    seed, step = 0x5EED0000 + i, 11 + i
    kw = {}
    if p > 0:
        kw = dict(p_ent=p, keep_cand=ko.dropout_keep_mask(seed, H.STREAM_CAND, step, N, d, p),
                  keep_po_ent=ko.dropout_keep_mask(seed, H.STREAM_PO_ENT, step, n_po, d, p),
                  keep_sp_ent=ko.dropout_keep_mask(seed, H.STREAM_SP_ENT, step, n_sp, d, p))
    ref = oracle_step(scorer, E, R, z, cand.astype(np.int32), y, loss, smoothing, **kw)
    batch = make_batch(z, cand.astype(np.int32), None, labels=y)
    if i % 3:
        batch.cand_ids, batch.cand_first, batch.n_cand = None, 2, N
    else:
        batch.cand_unique = bool(i % 2)
    if p > 0:
        batch.drop_cand = H.DropoutSpec(p, seed, H.STREAM_CAND, step)
        batch.drop_po_ent = H.DropoutSpec(p, seed, H.STREAM_PO_ENT, step)
        batch.drop_sp_ent = H.DropoutSpec(p, seed, H.STREAM_SP_ENT, step)
    if i % 4 == 3:
        monkeypatch.setenv("OKGE_GT_MBYTES", str(max(1, ((B + 63) // 64 * 64) * 64 * 4 * 256 // (1 << 20))))   # ranges of one round
    hp = H.HotPath("cuda:0")
    hp._ws, hp._ws_bytes = None, 0
    Et, Rt = dev(E), dev(R)
    dE, dR = torch.zeros_like(Et), torch.zeros_like(Rt)
    lossv = hp.forward_backward(Et, Rt, scorer, batch, dE, dR, loss=loss, label_smoothing=smoothing, grads_zero=bool(i % 2))
    torch.cuda.synchronize()
    info = dict(i=i, scorer=scorer, d=d, N=N, B=B, loss=loss, p=p)
    assert abs(lossv.item() - ref["loss"]) <= 5e-5 * abs(ref["loss"]) + 1e-5, (info, lossv.item(), ref["loss"])
    for mine, r in ((dE, ref["dE"]), (dR, ref["dR"])):
        np.testing.assert_allclose(mine.cpu().numpy(), r, rtol=0, atol=5e-5 * np.abs(r).max() + 5e-7, err_msg=str(info))


@pytest.mark.parametrize("i", range(24))
def test_random_ranks(okge_lib, i):
    """filtered ranks on random score matrices with forced ties, multi-mention groups, many groups per row, long filter
    lists, unaligned / long rows (register and streaming sweeps): bit-equal to the oracle's rule."""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(9100 + i)
    B = int(rng.integers(1, 40))
    N = int(rng.choice([5, 63, 64, 1000, 4099, 14541, 16384, 16385, 20011]))
    pad = int(rng.choice([0, 0, 1, 3]))                                  # leading dimension not a multiple of 4: scalar path
    x = np.round(rng.standard_normal((B, N)).astype(np.float32) * 2, int(rng.choice([0, 1, 3])))      # few decimals -> ties
    row_ptr, grp_ptr, ids, filt_ptr, filt_col = [0], [0], [], [0], []
    for b in range(B):
        for _ in range(int(rng.choice([1, 1, 2, 3, 9, 20, 70]))):
            ids += rng.integers(0, N, int(rng.integers(1, 4))).tolist()
            grp_ptr.append(len(ids))
        row_ptr.append(len(grp_ptr) - 1)
        nf = int(rng.choice([0, 3, 40, 300, 700]))
        filt_col += sorted(set(rng.integers(0, N, nf).tolist()))
        filt_ptr.append(len(filt_col))
    filt = np.zeros((B, N), bool)
    for b in range(B):
        filt[b, filt_col[filt_ptr[b]:filt_ptr[b + 1]]] = True
    ref = ko.filtered_ranks(x, filt, np.asarray(row_ptr), np.asarray(grp_ptr), np.asarray(ids, np.int32))
    ld = (N + 3) // 4 * 4 + pad
    buf = torch.zeros((B, ld), device="cuda:0")
    buf[:, :N] = torch.from_numpy(x).cuda()
    t = lambda a, dt: torch.tensor(a, dtype=dt, device="cuda:0")           # noqa: E731
    hp = H.HotPath("cuda:0")
    got = hp.filtered_ranks(buf[:, :N], t(filt_ptr, torch.int64), t(filt_col or [0], torch.int32), t(row_ptr, torch.int64),
                            t(grp_ptr, torch.int64), t(ids, torch.int32)).cpu().numpy()
    np.testing.assert_array_equal(got, ref)
    # the two-phase (sharded) form over 3 column shards gives the same ranks
    cuts = [0, N // 3, 2 * N // 3, N]
    parts = [buf[:, cuts[k]:cuts[k + 1]] for k in range(3) if cuts[k + 1] > cuts[k]]
    offs = [cuts[k] for k in range(3) if cuts[k + 1] > cuts[k]]
    rp, gp, idt, fp, fc = t(row_ptr, torch.int64), t(grp_ptr, torch.int64), t(ids, torch.int32), t(filt_ptr, torch.int64), t(filt_col or [0], torch.int32)
    true = torch.stack([hp.group_true_scores(p, o, rp, gp, idt) for p, o in zip(parts, offs)]).max(0).values
    counts = sum(hp.rank_counts(p, o, fp, fc, rp, true) for p, o in zip(parts, offs))
    np.testing.assert_array_equal((counts[:, 0] + counts[:, 1] // 2).cpu().numpy(), ref)
