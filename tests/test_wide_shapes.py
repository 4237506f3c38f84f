"""The wide path (slot sizes 513 .. 4096: csrc/okge_wide.hip, wide_core in csrc/okge_api_train.hip) on the GPU against float64, at the
smallest shapes at which it can go wrong.  Truth and fp32 yardstick: tests/wide_reference.py (pinned by test_wide_reference.py);
rule: lstm_reference.band_check -- per |want| band max error <= 3 x and rms error <= 1.6 x the fp32 restatement's error against
float64, floor 1e-7 max|want| -- on scores, dE and dR; the loss within 3e-5 relative (test_hip_parity.py's bound).

Measured on an MI355X (worst ratio to the fp32 restatement over all cases of test_step_against_float64, and the failures, if
any): profiles/wide.md."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_reference as wr  # noqa: E402
from lstm_reference import band_check  # noqa: E402
from oracle import kge_oracle as ko  # noqa: E402

pytestmark = pytest.mark.gpu
SEED, STEP = 0xC0FFEE1234, 5


@pytest.fixture(scope="module")
def hp():
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    return HotPath("cuda:0")


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to("cuda:0")


def problem(seed, d, n_po, n_sp, N, mode, max_pos=4):
    """tables, ids, candidate list and labels.  mode: 'range' (ids 2 .. N + 1), 'unique' (N distinct ids in any order),
    'dup' (N positions over about N / 12 distinct ids)"""
    rng = np.random.default_rng(seed)
    n_ent = {"range": N + 2, "unique": N + 9, "dup": max(4, N // 12 + 3) + 2}[mode]
    n_rel = 7
    std = 0.3 if d <= 1024 else 0.2
    E, R = (rng.standard_normal((n_ent, d)) * std).astype(np.float32), (rng.standard_normal((n_rel, d)) * std).astype(np.float32)
    z = {}
    if n_po:
        z["po_rel"], z["po_obj"] = rng.integers(2, n_rel, n_po).astype(np.int32), rng.integers(2, n_ent, n_po).astype(np.int32)
    if n_sp:
        z["sp_subj"], z["sp_rel"] = rng.integers(2, n_ent, n_sp).astype(np.int32), rng.integers(2, n_rel, n_sp).astype(np.int32)
    if mode == "range":
        cand = np.arange(2, n_ent)
    elif mode == "unique":
        cand = rng.permutation(np.arange(2, n_ent))[:N]
    else:
        cand = rng.integers(2, n_ent, N)
    y = np.zeros((n_po + n_sp, N), np.float32)
    for b in range(n_po + n_sp):
        y[b, rng.choice(N, size=int(rng.integers(1, min(max_pos, N) + 1)), replace=False)] = 1
    return E, R, z, cand.astype(np.int32), y


def make_batch(z, cand, mode, y, drop=None, p_ent=0.0, p_rel=0.0, masks=None):
    """drop: None, 'philox' (the kernels draw the masks) or 'keep' (explicit masks = `masks`)"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    b = H.PrefixBatch()
    if "po_rel" in z:
        b.po_rel, b.po_obj = dev(z["po_rel"]), dev(z["po_obj"])
    if "sp_subj" in z:
        b.sp_subj, b.sp_rel = dev(z["sp_subj"]), dev(z["sp_rel"])
    if mode == "range":
        b.cand_first, b.n_cand = int(cand[0]), len(cand)
    else:
        b.cand_ids, b.n_cand, b.cand_unique = dev(cand), len(cand), mode == "unique"
    if y is not None:
        b.pos_row, b.pos_col = H.positives_from_dense(dev(y))
    if drop is not None:
        for attr, key, stream, p in (("drop_cand", "keep_cand", H.STREAM_CAND, p_ent), ("drop_po_ent", "keep_po_ent", H.STREAM_PO_ENT, p_ent),
                                     ("drop_po_rel", "keep_po_rel", H.STREAM_PO_REL, p_rel), ("drop_sp_ent", "keep_sp_ent", H.STREAM_SP_ENT, p_ent),
                                     ("drop_sp_rel", "keep_sp_rel", H.STREAM_SP_REL, p_rel)):
            if p <= 0 or masks.get(key) is None:
                continue
            setattr(b, attr, H.DropoutSpec(p, SEED, stream, STEP) if drop == "philox" else H.DropoutSpec(p=p, keep=dev(masks[key].astype(np.uint8))))
    return b


def padded_scores(B, N, extra=5):
    """a NaN-filled (B, N + extra) block and its (B, N) view: what lies behind the leading dimension must stay NaN"""
    buf = torch.full((B, N + extra), float("nan"), device="cuda:0")
    return buf, buf[:, :N]


# scorer, d, n_po, n_sp, N, candidates, loss, smoothing, grads_zero, dropout
CASES = [
    ("distmult", 513, 1, 0, 1, "range", "bce", 0.0, True, None),            # odd, first wide width; one row, one candidate
    ("complex", 514, 0, 1, 63, "unique", "kl", 0.0, False, None),           # halves of 257; sp only
    ("complex", 528, 31, 32, 64, "range", "bce", 0.1, True, "philox"),
    ("complex", 1000, 32, 32, 65, "dup", "bce", 0.0, False, None),          # half 500, a partial last chunk; repeated ids: atomics
    ("complex", 1024, 33, 32, 129, "range", "kl", 0.0, True, "keep"),
    ("distmult", 520, 31, 32, 129, "dup", "kl", 0.0, True, "philox"),
    ("distmult", 4096, 70, 61, 700, "unique", "bce", 0.1, True, None),      # two row blocks, six tiles
    ("complex", 4096, 70, 61, 700, "range", "kl", 0.0, False, "philox"),
    ("distmult", 1024, 70, 61, 700, "range", "bce", 0.0, False, "keep"),    # a table slice with dropout, accumulated
]


def run_case(hp, case, seed, monkeypatch=None, gt_mbytes=None):
    scorer, d, n_po, n_sp, N, mode, loss, smoothing, grads_zero, drop = case
    E, R, z, cand, y = problem(seed, d, n_po, n_sp, N, mode)
    p_ent, p_rel = (0.4, 0.25) if drop else (0.0, 0.0)
    masks = None
    if drop == "philox":
        masks = wr.philox_masks(SEED, STEP, n_po, n_sp, N, d, p_ent, p_rel)
    elif drop == "keep":
        rng = np.random.default_rng(seed + 1)
        masks = {k: (rng.random((n, d)) >= p) if n else None for k, n, p in (("keep_cand", N, p_ent), ("keep_po_ent", n_po, p_ent),
                 ("keep_po_rel", n_po, p_rel), ("keep_sp_ent", n_sp, p_ent), ("keep_sp_rel", n_sp, p_rel))}
    rng = np.random.default_rng(seed + 2)
    dE0 = np.zeros_like(E) if grads_zero else (rng.standard_normal(E.shape) * 1e-4).astype(np.float32)
    dR0 = np.zeros_like(R) if grads_zero else (rng.standard_normal(R.shape) * 1e-4).astype(np.float32)
    t = wr.truth(scorer, E, R, z, cand, y, loss, smoothing, p_ent, p_rel, masks)
    yd = wr.yardstick(scorer, E, R, z, cand, y, loss, smoothing, p_ent, p_rel, masks, gt_mbytes=gt_mbytes, dE0=dE0, dR0=dR0)
    want = dict(outputs=t["outputs"], dE=dE0.astype(np.float64) + t["dE"], dR=dR0.astype(np.float64) + t["dR"], loss=t["loss"])
    if monkeypatch is not None:
        monkeypatch.delenv("OKGE_GT_MBYTES", raising=False)
        if gt_mbytes is not None:
            monkeypatch.setenv("OKGE_GT_MBYTES", str(gt_mbytes))
    batch = make_batch(z, cand, mode, y, drop, p_ent, p_rel, masks)
    Et, Rt, dE, dR = dev(E), dev(R), dev(dE0), dev(dR0)
    buf, scores = padded_scores(n_po + n_sp, N)
    loss_dev = hp.forward_backward(Et, Rt, scorer, batch, dE, dR, loss=loss, label_smoothing=smoothing, scores=scores, grads_zero=grads_zero)
    torch.cuda.synchronize()
    assert torch.isnan(buf[:, N:]).all()                                    # nothing behind the leading dimension was written
    got = dict(outputs=scores.cpu().numpy(), dE=dE.cpu().numpy(), dR=dR.cpu().numpy(), loss=loss_dev.item())
    return got, want, yd, (Et, Rt, batch)


def check_bands(tag, got, want, yd):
    worst = {}
    for k in ("outputs", "dE", "dR"):
        worst[k] = band_check(f"{tag}:{k}", got[k], want[k], yd[k])
    print(f"wide-bands {tag} loss_rel={abs(got['loss'] - want['loss']) / abs(want['loss']):.2e} " +
          " ".join(f"{k}=max{w[0]:.2f}/rms{w[1]:.2f}" for k, w in worst.items()))
    assert abs(got["loss"] - want["loss"]) <= 3e-5 * abs(want["loss"]), (tag, got["loss"], want["loss"])
    return worst


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-d{c[1]}-b{c[2]}+{c[3]}-n{c[4]}-{c[5]}-{c[6]}{'-drop_' + c[9] if c[9] else ''}" for c in CASES])
def test_step_against_float64(hp, case, monkeypatch):
    got, want, yd, _ = run_case(hp, case, 300 + CASES.index(case), monkeypatch)
    check_bands("-".join(str(c) for c in case[:7]), got, want, yd)


def test_loss_only_touches_no_gradient(hp, monkeypatch):
    case = ("complex", 528, 31, 32, 129, "range", "kl", 0.0, True, None)
    scorer, d, n_po, n_sp, N, mode, loss, smoothing, _, _ = case
    E, R, z, cand, y = problem(41, d, n_po, n_sp, N, mode)
    t = wr.truth(scorer, E, R, z, cand, y, loss, smoothing)
    monkeypatch.delenv("OKGE_GT_MBYTES", raising=False)
    out = hp.forward_backward(dev(E), dev(R), scorer, make_batch(z, cand, mode, y), None, None, loss=loss, loss_only=True)
    assert abs(out.item() - t["loss"]) <= 3e-5 * abs(t["loss"])


def test_clear_grads_from_nan_buffers(hp, monkeypatch):
    """OKGE_TRAIN_CLEAR_GRADS: gradient buffers full of NaN on entry; exact zeros where nothing was added, no NaN anywhere"""
    monkeypatch.delenv("OKGE_GT_MBYTES", raising=False)
    d, n_po, n_sp, N = 520, 5, 4, 130
    E, R, z, cand, y = problem(51, d, n_po, n_sp, N + 6, "range")
    cand, y = cand[3:3 + N], y[:, :N]                                        # rows in front of AND behind the candidate range
    z["po_obj"][:], z["sp_subj"][:] = cand[1], cand[2]                      # prefix entities inside the range: the rest stays clear
    z["po_rel"][:], z["sp_rel"][:] = 3, 4
    masks = wr.philox_masks(SEED, STEP, n_po, n_sp, N, d, 0.4, 0.0)
    t = wr.truth("complex", E, R, z, cand, y, "bce", 0.0, 0.4, 0.0, masks)
    yd = wr.yardstick("complex", E, R, z, cand, y, "bce", 0.0, 0.4, 0.0, masks)
    batch = make_batch(z, cand, "range", y, "philox", 0.4, 0.0, masks)
    dE, dR = torch.full(E.shape, float("nan"), device="cuda:0"), torch.full(R.shape, float("nan"), device="cuda:0")
    loss = hp.forward_backward(dev(E), dev(R), "complex", batch, dE, dR, clear_grads=True)
    torch.cuda.synchronize()
    gE, gR = dE.cpu().numpy(), dR.cpu().numpy()
    assert np.isfinite(gE).all() and np.isfinite(gR).all()
    outside = np.setdiff1d(np.arange(E.shape[0]), cand)
    assert len(outside) == 8 and not gE[outside].any() and not gR[[0, 1, 2, 5, 6]].any()
    assert not gE[cand][~masks["keep_cand"] & (np.arange(N)[:, None] != 1) & (np.arange(N)[:, None] != 2)].any()     # dropped columns
    check_bands("clear_grads", dict(outputs=t["outputs"], dE=gE, dR=gR, loss=loss.item()), t, yd)


def test_ranges_do_not_change_a_score_bit(hp, monkeypatch):
    """OKGE_GT_MBYTES = 1 at d = 4096, B = 131, N = 700: six one-tile ranges.  The score block is bit-identical to the one-range
    run and to okge_score_prefixes into a block with another leading dimension; the gradients pass the same bands."""
    case = ("complex", 4096, 70, 61, 700, "range", "bce", 0.0, True, "philox")
    assert wr.plan(131, 700, 4096, 1)["n_ranges"] == 6 and wr.plan(131, 700, 4096)["n_ranges"] == 1
    one, want, yd1, _ = run_case(hp, case, 77, monkeypatch)
    many, _, ydm, (Et, Rt, batch) = run_case(hp, case, 77, monkeypatch, gt_mbytes=1)
    assert np.array_equal(one["outputs"], many["outputs"])
    buf, view = padded_scores(131, 700, extra=13)
    hp.score(Et, Rt, "complex", batch, out=view)
    torch.cuda.synchronize()
    assert np.array_equal(view.cpu().numpy(), one["outputs"]) and torch.isnan(buf[:, 700:]).all()
    check_bands("ranges-1", one, want, yd1)
    check_bands("ranges-6", many, want, ydm)
    # the KL statistics pass over several ranges too
    kl = ("distmult", 1024, 33, 32, 700, "unique", "kl", 0.0, True, None)
    got, want, yd, _ = run_case(hp, kl, 78, monkeypatch, gt_mbytes=1)
    assert wr.plan(65, 700, 1024, 1)["n_ranges"] > 1
    check_bands("ranges-kl", got, want, yd)


def test_unit_table_copies_query_elements(hp):
    """candidate rows with a single 1.0: every score IS one element of the query, bit for bit -- at the first and last column
    of a chunk, of the vector / scalar tail, and on both sides of a tile edge (N = 130).  The relation rows are the unit of the
    fold (ones; ComplEx: real part one, imaginary part zero), so the query IS the prefix entity row whatever the fold rounds."""
    for scorer, d in (("distmult", 513), ("complex", 1000), ("distmult", 4096)):
        E, R, z, _, _ = problem(61, d, 3, 2, 40, "range")
        R[:] = 1.0
        if scorer == "complex":
            R[:, d // 2:] = 0.0
        cols = np.array([0, 1, 7, 8, 15, 16, 17, 31, 32, 255, 256, 511, 512, d - 17, d - 16, d - 9, d - 8, d - 2, d - 1])
        cols = np.concatenate([cols, np.random.default_rng(1).integers(0, d, 130 - len(cols))])
        T = np.zeros((130, d), np.float32)
        T[np.arange(130), cols] = 1.0
        b = make_batch(z, np.arange(130), "range", None)
        b.cand_first, b.cand_table = 0, dev(T)
        out = hp.score(dev(E), dev(R), scorer, b).cpu().numpy()
        q = E[np.concatenate([z["po_obj"], z["sp_subj"]])]
        assert np.array_equal(out, q[:, cols]), (scorer, d)


def test_nan_around_every_buffer_and_exact_workspace(hp, okge_lib, monkeypatch):
    """NaN past the last table row, in the unused workspace and around a workspace of exactly the asked size never reaches an
    output; the sentinels around that workspace survive; two runs give the same bits; one byte less answers -3"""
    monkeypatch.delenv("OKGE_GT_MBYTES", raising=False)
    from open_knowledge_graph_embeddings_amd import _native as N_
    d, n_po, n_sp, N = 1000, 33, 32, 129
    E, R, z, cand, y = problem(71, d, n_po, n_sp, N, "unique")
    Ebig, Rbig = torch.full((E.shape[0] + 3, d), float("nan"), device="cuda:0"), torch.full((R.shape[0] + 3, d), float("nan"), device="cuda:0")
    Ebig[:E.shape[0]] = dev(E)
    Rbig[:R.shape[0]] = dev(R)
    Et, Rt = Ebig[:E.shape[0]], Rbig[:R.shape[0]]
    batch = make_batch(z, cand, "unique", y)
    need = int(okge_lib.okge_train_workspace_bytes(n_po + n_sp, N, d))
    assert need > 0 and need % 256 == 0
    guard = 4096
    raw = torch.full(((need + 2 * guard) // 4,), float("nan"), device="cuda:0")
    ws_ptr = raw.data_ptr() + guard

    def call(ws_bytes, kind="kl"):
        pb, c, keep = hp._batch(batch)
        t = hp._tables(Et, Rt, "complex")
        pos, keep_pos = hp._positives(batch)
        dE, dR = torch.zeros_like(Et), torch.zeros_like(Rt)
        _, sc = padded_scores(n_po + n_sp, N)
        loss = torch.zeros(1, dtype=torch.float64, device="cuda:0")
        rc = okge_lib.okge_train_forward_backward(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), ctypes.byref(pos), N_.LOSSES[kind], 0.0,
                                                  float((n_po + n_sp) * N), N_.OKGE_TRAIN_GRADS_ZERO | N_.OKGE_TRAIN_UNIQUE_CANDIDATES,
                                                  loss.data_ptr(), dE.data_ptr(), dR.data_ptr(), sc.data_ptr(), sc.stride(0),
                                                  ctypes.c_void_p(ws_ptr), ctypes.c_size_t(ws_bytes), hp._stream())
        torch.cuda.synchronize()
        return rc, loss.item(), sc.cpu().numpy(), dE.cpu().numpy(), dR.cpu().numpy()

    assert call(need - 1)[0] == -3
    assert torch.isnan(raw).all()                                             # refused before any launch
    for kind in ("kl", "bce"):
        raw.fill_(float("nan"))
        rc, loss, sc, gE, gR = call(need, kind)
        assert rc == 0
        assert np.isfinite(loss) and np.isfinite(sc).all() and np.isfinite(gE).all() and np.isfinite(gR).all()
        assert torch.isnan(raw[:guard // 4]).all() and torch.isnan(raw[(guard + need) // 4:]).all()      # the sentinels survive
        t = wr.truth("complex", E, R, z, cand, y, kind)
        assert abs(loss - t["loss"]) <= 3e-5 * abs(t["loss"])
        rc2, loss2, sc2, gE2, gR2 = call(need, kind)
        assert rc2 == 0 and loss2 == loss and np.array_equal(sc2, sc)         # (the prefix rows' gradients are float atomics)
        assert np.abs(gE2 - gE).max() <= 2e-6 * np.abs(gE).max() and np.abs(gR2 - gR).max() <= 2e-6 * np.abs(gR).max()


def test_statuses_before_any_launch(hp, okge_lib):
    """d = 4097 answers -2; what stays refused above 512 answers -2 at d = 520 (okge.h / DESIGN section 9)"""
    from open_knowledge_graph_embeddings_amd import _native as N_
    from open_knowledge_graph_embeddings_amd import hotpath as H

    def refused(fn, *a, **kw):
        with pytest.raises(N_.OkgeError) as ei:
            fn(*a, **kw)
        assert "code -2" in str(ei.value), str(ei.value)
        return str(ei.value)

    for d, scorers in ((4097, ("distmult",)), (4098, ("complex",))):
        E, R, z, cand, y = problem(81, d, 2, 2, 10, "range")
        for s in scorers:
            b = make_batch(z, cand, "range", y)
            ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
            pb, c, keep = hp._batch(b)
            t = hp._tables(dev(E), dev(R), s)
            out = torch.zeros((4, 12), device="cuda:0")
            assert okge_lib.okge_score_prefixes(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), out.data_ptr(), 12, ws.data_ptr(), 1 << 20,
                                                hp._stream()) == -2
            assert b"4096" in okge_lib.okge_last_error()                          # the message names the new limit
            assert not out.any()
    d = 520
    E, R, z, cand, y = problem(82, d, 3, 2, 30, "range")
    Et, Rt = dev(E), dev(R)
    b = make_batch(z, cand, "range", y)
    # the row-sparse step
    pb, c, keep = hp._batch(b)
    t = hp._tables(Et, Rt, "complex")
    pos, keep_pos = hp._positives(b)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda:0")
    loss = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    dEr, dRr = torch.zeros((30 + 5, d), device="cuda:0"), torch.zeros((5, d), device="cuda:0")
    assert okge_lib.okge_train_forward_backward(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), ctypes.byref(pos), 0, 0.0, 150.0,
                                                N_.OKGE_TRAIN_ROW_GRADS, loss.data_ptr(), dEr.data_ptr(), dRr.data_ptr(), None, 0,
                                                ws.data_ptr(), 64 << 20, hp._stream()) == -2
    assert okge_lib.okge_train_row_grads_workspace_bytes(5, 30, d) == 0
    # the data-bias scorers
    refused(hp.score, Et, Rt, "bias_entity", b)
    # the sharded phases
    sh = H.Shard(0, E.shape[0], 0)
    Q = torch.zeros((64, 512), device="cuda:0")
    refused(hp.encode_queries, Et, Rt, "complex", b, sh)
    refused(hp.score_queries, Et, Rt, "complex", Q, 5, b, sh)
    refused(hp.row_logsumexp, Et, Rt, "complex", Q, 5, b, sh)
    refused(hp.train_tiles, Et, Rt, "complex", Q, b, sh, torch.zeros_like(Et), torch.zeros_like(Q), 30)
    # top-k and the fused evaluation
    refused(hp.topk_prefixes, Et, Rt, "complex", make_batch(z, cand, "range", None), 3)
    filt_ptr = torch.zeros(6, dtype=torch.int64, device="cuda:0")
    row_ptr = torch.arange(6, dtype=torch.int64, device="cuda:0")
    ids = torch.zeros(5, dtype=torch.int32, device="cuda:0")
    refused(hp.evaluate_fused, Et, Rt, "complex", make_batch(z, cand, "range", None), filt_ptr, torch.zeros(1, dtype=torch.int32, device="cuda:0"),
            row_ptr, row_ptr, ids)


# ------------------------------------------------------------------------------------------------------- evaluation
def _eval_case(rng, n_ent, n_rel, n_po, n_sp, cand_list):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    from open_knowledge_graph_embeddings_amd.dataset import CollatedBatch
    batch = H.PrefixBatch()
    if n_po:
        batch.po_rel, batch.po_obj = dev(rng.integers(2, n_rel, n_po).astype(np.int32)), dev(rng.integers(2, n_ent, n_po).astype(np.int32))
    if n_sp:
        batch.sp_subj, batch.sp_rel = dev(rng.integers(2, n_ent, n_sp).astype(np.int32)), dev(rng.integers(2, n_rel, n_sp).astype(np.int32))
    if cand_list:
        cand = rng.permutation(np.arange(2, n_ent))[:(n_ent - 2) // 2].astype(np.int32)
        batch.cand_ids, N = dev(cand), len(cand)
    else:
        batch.cand_first, batch.n_cand, N = 2, n_ent - 2, n_ent - 2
    row_ptr, grp_ptr, ids, filt_ptr, filt_col = [0], [0], [], [0], []
    for b in range(n_po + n_sp):
        row_ids = []
        for _ in range(int(rng.integers(0, 4))):
            g = rng.integers(0, N, int(rng.integers(1, 4))).tolist()
            ids.extend(g)
            row_ids.extend(g)
            grp_ptr.append(len(ids))
        row_ptr.append(len(grp_ptr) - 1)
        f = np.unique(np.concatenate([rng.integers(0, N, int(rng.integers(0, 12))), np.asarray(row_ids, np.int64)])).astype(np.int64)
        filt_col.extend(f.tolist())
        filt_ptr.append(len(filt_col))
    csr = dict(filt_ptr=np.asarray(filt_ptr, np.int64), filt_col=np.asarray(filt_col, np.int32), row_ptr=np.asarray(row_ptr, np.int64),
               grp_ptr=np.asarray(grp_ptr, np.int64), ids=np.asarray(ids, np.int32))
    dd = {k: dev(v) for k, v in csr.items()}
    return CollatedBatch(batch, 1.0, 1.0, N, row_ptr=dd["row_ptr"], grp_ptr=dd["grp_ptr"], ids=dd["ids"], filt_ptr=dd["filt_ptr"],
                         filt_col=dd["filt_col"]), csr, N


@pytest.mark.parametrize("scorer,d", [("distmult", 520), ("complex", 1024)])
def test_pipelined_evaluator(hp, scorer, d):
    """PipelinedEvaluator (okge_evaluate_batch = the wide score + the d-agnostic ranks and meters): ranks bit-equal to the oracle's
    rule applied to the kernel's own score block, meters equal to metrics_from_ranks; FusedEvaluator refuses at construction"""
    from open_knowledge_graph_embeddings_amd.evaluate import FusedEvaluator, PipelinedEvaluator
    rng = np.random.default_rng(d)
    n_ent, n_rel = 263, 9
    E, R = (rng.standard_normal((n_ent, d)) * 0.3).astype(np.float32), (rng.standard_normal((n_rel, d)) * 0.3).astype(np.float32)
    Et, Rt = dev(E), dev(R)
    cases = [_eval_case(rng, n_ent, n_rel, 33, 32, False), _eval_case(rng, n_ent, n_rel, 0, 70, True), _eval_case(rng, n_ent, n_rel, 5, 0, False)]
    ev = PipelinedEvaluator(Et, Rt, scorer, collect_ranks=True)
    meters, n = ev.run([c[0] for c in cases])
    want = []
    for cb, csr, N in cases:
        x = hp.score(Et, Rt, scorer, cb.batch).cpu().numpy()
        filt = np.zeros((cb.batch.B, N), bool)
        for b in range(cb.batch.B):
            filt[b, csr["filt_col"][csr["filt_ptr"][b]:csr["filt_ptr"][b + 1]]] = True
        want.append(ko.filtered_ranks(x, filt, csr["row_ptr"], csr["grp_ptr"], csr["ids"]))
    want = np.concatenate(want)
    assert n == len(want) > 0
    np.testing.assert_array_equal(ev.ranks.cpu().numpy(), want)
    m, _ = ko.metrics_from_ranks(want, None)
    for k in ("mrr", "mr", "h1", "h3", "h10", "h50"):
        assert abs(meters[k].avg - m[k]) <= 1e-6 * max(1.0, abs(m[k])), k
    with pytest.raises(NotImplementedError, match="PipelinedEvaluator"):
        FusedEvaluator(Et, Rt, scorer)


# ------------------------------------------------------------------------------------------------------------- steps
def _step_problems(k, d, n_ent, n_rel, n_po, n_sp, n_cand=None, seed=900):
    """k batches on one pair of tables; n_cand: a unique sampled list per batch (None: 1-vs-all)"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    rng = np.random.default_rng(seed)
    E, R = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32), (rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)
    out = []
    for _ in range(k):
        cand = np.arange(2, n_ent) if n_cand is None else rng.permutation(np.arange(2, n_ent))[:n_cand]
        po = (rng.integers(2, n_rel, n_po).astype(np.int32), rng.integers(2, n_ent, n_po).astype(np.int32))
        sp = (rng.integers(2, n_ent, n_sp).astype(np.int32), rng.integers(2, n_rel, n_sp).astype(np.int32))
        y = np.zeros((n_po + n_sp, len(cand)), np.float32)
        for r in range(n_po + n_sp):
            y[r, rng.choice(len(cand), size=int(rng.integers(1, 4)), replace=False)] = 1
        pr, pc = H.positives_from_dense(dev(y))
        b = H.PrefixBatch(po_rel=dev(po[0]), po_obj=dev(po[1]), sp_subj=dev(sp[0]), sp_rel=dev(sp[1]), pos_row=pr, pos_col=pc)
        if n_cand is None:
            b.cand_first, b.n_cand = 2, n_ent - 2
        else:
            b.cand_ids, b.n_cand, b.cand_unique = dev(cand.astype(np.int32)), len(cand), True
        out.append((b, po, sp, cand, y))
    return E, R, out


def test_fused_step_with_clip_and_accumulation_against_the_oracle(okge_lib):
    """FusedTrainStep at d = 1024: three optimizer steps, each the clipped sum of two batches' gradients (accumulate = 2,
    grad_clip), against three oracle steps (float64 gradients, adagrad_step) under the G3 rule of
    test_hip_parity.test_g3_adagrad_steps: each step restarted from the state it is compared with, every element within
    test_oracle_golden.adagrad_tol, 97 % within 2e-6, the accumulators' roots within 1e-4"""
    from test_oracle_golden import adagrad_tol
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep
    d, n_ent, n_rel, lr, eps = 1024, 202, 8, 0.3, 1e-8
    E, R, probs = _step_problems(6, d, n_ent, n_rel, 20, 17)
    clip = 0.002
    ts = FusedTrainStep(dev(E), dev(R), "complex", lr=lr, grad_clip=clip, accumulate=2)
    with pytest.raises(NotImplementedError, match="dense gradients"):
        FusedTrainStep(dev(E), dev(R), "complex", weight_decay=0.0, sparse=True)
    for s in range(3):
        Eo, Ro, sE, sR = (x.cpu().numpy().copy() for x in (ts.E, ts.R, ts.sumE, ts.sumR))      # restart from the step's own state
        pE, pR = sE.copy(), sR.copy()
        gE, gR = np.zeros(E.shape), np.zeros(R.shape)
        for b, po, sp, cand, y in probs[2 * s:2 * s + 2]:
            ref = ko.step_forward_backward(ko.COMPLEX, Eo.astype(np.float64), Ro.astype(np.float64), po, sp, cand, y.astype(np.float64))
            gE, gR = gE + ref["dE"], gR + ref["dR"]
            loss = float(ts.step(b)[0])
            assert abs(loss - ref["loss"]) <= 3e-5 * abs(ref["loss"])
        norm = np.sqrt((gE ** 2).sum() + (gR ** 2).sum())
        assert norm > clip                                           # the clip bites
        coef = min(1.0, clip / (norm + 1e-6))
        ko.adagrad_step(Eo, (gE * coef).astype(np.float32), sE, lr)
        ko.adagrad_step(Ro, (gR * coef).astype(np.float32), sR, lr)
        torch.cuda.synchronize()
        for mine, ref_, s_mine, s_ref, s_prev in ((ts.E, Eo, ts.sumE, sE, pE), (ts.R, Ro, ts.sumR, sR, pR)):
            tol = adagrad_tol(s_ref, s_prev, lr, eps)
            diff = np.abs(mine.cpu().numpy() - ref_)
            print(f"wide-g3 step {s}: max diff / tol = {float((diff / tol).max()):.3f}, within 2e-6: {np.mean(diff <= 2e-6):.4f}")
            assert np.all(diff <= tol), float((diff / tol).max())
            assert np.mean(diff <= 2e-6) > 0.97
            np.testing.assert_allclose(np.sqrt(s_mine.cpu().numpy()), np.sqrt(s_ref), rtol=1e-4, atol=1e-6 * np.sqrt(s_ref.max()))


def test_graphed_step_equals_the_eager_step(okge_lib):
    """ten steps under GraphedTrainStep against FusedTrainStep at d = 1024, input dropout 0.4.  Unique sampled candidates and
    distinct prefix ids leave no float atomic on any path that writes a row once; the prefix rows still go through atomicAdd
    (one add per element onto a cleared buffer or an exclusive row: order-free), so the two walks are bit-equal"""
    from open_knowledge_graph_embeddings_amd.train_step import FusedTrainStep, GraphedTrainStep
    from open_knowledge_graph_embeddings_amd import hotpath as H
    d, n_ent, n_rel, n_po, n_sp = 1024, 300, 80, 20, 17
    E, R, probs = _step_problems(4, d, n_ent, n_rel, n_po, n_sp, n_cand=150, seed=901)
    rng = np.random.default_rng(3)
    batches = []
    for b, po, sp, cand, y in probs:                                  # distinct prefix ids, none of them a candidate
        free = np.setdiff1d(np.arange(2, n_ent), cand)
        ent = rng.permutation(free)[:n_po + n_sp].astype(np.int32)
        rel = rng.permutation(np.arange(2, n_rel))[:n_po + n_sp].astype(np.int32)
        b.po_obj, b.sp_subj, b.po_rel, b.sp_rel = dev(ent[:n_po]), dev(ent[n_po:]), dev(rel[:n_po]), dev(rel[n_po:])
        batches.append(b)
    plain = FusedTrainStep(dev(E.copy()), dev(R.copy()), "complex", lr=0.3, input_dropout=0.4, seed=77)
    inner = FusedTrainStep(dev(E.copy()), dev(R.copy()), "complex", lr=0.3, input_dropout=0.4, seed=77)
    graphed = GraphedTrainStep(inner, batches[0], pos_capacity=max(b.nnz for b in batches) + 7)
    np.testing.assert_array_equal(inner.E.cpu().numpy(), E)
    for i in range(10):
        lp, lg = float(plain.step(batches[i % 4])[0]), float(graphed.step(batches[i % 4])[0])
        assert lp == lg, (i, lp, lg)
    assert torch.equal(inner.E, plain.E) and torch.equal(inner.R, plain.R) and torch.equal(inner.sumE, plain.sumE)
    assert H is not None
    # 1-vs-all with repeated prefix ids: the prefix rows' gradients are float atomics, so a step's gradients agree to 2e-6 of
    # their largest.  Adagrad's first steps divide by |g|: where |g| is of the size of that noise the TABLES move apart by far
    # more (test_oracle_golden.adagrad_tol), and so would every later gradient.  So each of the ten replays is compared with the
    # eager step FROM THE SAME STATE: the eager step's tables and accumulators are set to the graphed ones after every step.
    E2, R2, probs2 = _step_problems(3, d, 200, 6, 20, 17, seed=902)
    p2 = FusedTrainStep(dev(E2.copy()), dev(R2.copy()), "complex", lr=0.3, input_dropout=0.4, seed=5)
    i2 = FusedTrainStep(dev(E2.copy()), dev(R2.copy()), "complex", lr=0.3, input_dropout=0.4, seed=5)
    g2 = GraphedTrainStep(i2, probs2[0][0], pos_capacity=max(p[0].nnz for p in probs2) + 3)
    for i in range(10):
        lp, lg = float(p2.step(probs2[i % 3][0])[0]), float(g2.step(probs2[i % 3][0])[0])
        assert abs(lp - lg) <= 1e-7 * abs(lp), (i, lp, lg)
        # (a 1-vs-all step leaves its entity gradient in place: the next one overwrites it)
        assert float((p2.dE - i2.dE).abs().max()) <= 2e-6 * float(p2.dE.abs().max()), i
        for mine, theirs in ((p2.E, i2.E), (p2.R, i2.R), (p2.sumE, i2.sumE), (p2.sumR, i2.sumR)):
            assert float((mine - theirs).abs().max()) < 5e-3
            mine.copy_(theirs)


def _lookup_model(E, R, scorer):
    from open_knowledge_graph_embeddings_amd.dataset import EntityRelationDatasetMeta
    from open_knowledge_graph_embeddings_amd.model import Models
    name = "LookupComplexRelationModel" if scorer == "complex" else "LookupDistmultRelationModel"
    m = getattr(Models, name)(entity_slot_size=E.shape[1], input_dropout=0.0, init_std=0.1, sparse=False,
                              train_data=EntityRelationDatasetMeta(entities_size=E.shape[0], relations_size=R.shape[0])).cuda()
    m.entity_embedding.weight.data.copy_(dev(E))
    m.relation_embedding.weight.data.copy_(dev(R))
    return m


def test_addloss_module_and_okge_adagrad(okge_lib):
    """the drop-in path at d = 1024: AddLossModule (no training outputs) + OkgeAdagrad against the oracle's step and update,
    at the tolerances of test_dropin_path.test_addloss_without_training_outputs_and_okge_adagrad_step"""
    from open_knowledge_graph_embeddings_amd.optim import OkgeAdagrad
    from open_knowledge_graph_embeddings_amd.trainer import AddLossModule
    E, R, probs = _step_problems(1, 1024, 150, 7, 6, 7, seed=903)
    b, po, sp, cand, y = probs[0]
    ref = ko.step_forward_backward(ko.COMPLEX, E, R, po, sp, cand, y)
    m = _lookup_model(E, R, "complex")
    m.train()
    mod = AddLossModule(m, torch.nn.BCEWithLogitsLoss(reduction="sum"), 0.0, training_outputs=False)
    opt = OkgeAdagrad(torch.optim.Adam(m.parameters(), lr=0).param_groups)
    for grp in opt.param_groups:
        grp["lr"], grp["weight_decay"] = 0.3, 1e-10
    col = lambda a: dev(np.asarray(a, np.int32).reshape(-1, 1))       # noqa: E731
    loss, hook, outs = mod(inputs=[(col(po[0]), col(po[1])), (col(sp[0]), col(sp[1]))], labels=dev(y), use_batch_shared_entities=False,
                           batch_shared_entities=col(cand), epoch=1, input_style_triple_or_prefix="right_and_left_prefix")
    assert outs is None and hook is None
    assert abs(float(loss.detach()) - ref["loss"]) <= 3e-5 * abs(ref["loss"])
    (loss.sum() / float(y.size)).backward()
    gE, gR = m.entity_embedding.weight.grad, m.relation_embedding.weight.grad
    np.testing.assert_allclose(gE.cpu().numpy(), ref["dE"], rtol=0, atol=3e-5 * np.abs(ref["dE"]).max())
    np.testing.assert_allclose(gR.cpu().numpy(), ref["dR"], rtol=0, atol=3e-5 * np.abs(ref["dR"]).max())
    Eo, Ro = E.copy(), R.copy()
    ko.adagrad_step(Eo, gE.cpu().numpy(), np.zeros_like(E), 0.3)
    ko.adagrad_step(Ro, gR.cpu().numpy(), np.zeros_like(R), 0.3)
    opt.step()
    np.testing.assert_allclose(m.entity_embedding.weight.detach().cpu().numpy(), Eo, rtol=0, atol=2e-6)
    np.testing.assert_allclose(m.relation_embedding.weight.detach().cpu().numpy(), Ro, rtol=0, atol=2e-6)


@pytest.mark.parametrize("scorer,d", [("complex", 1024), ("distmult", 513)])
def test_model_methods_with_gradients_against_the_cpu_twin(okge_lib, scorer, d):
    """sp_prefix_score / po_prefix_score / triple_score with gradients enabled (forward: the wide score on encoded rows; backward:
    okge_prefix_score_backward) against torch autograd on the float64 twin: test_autograd_surface's tolerances"""
    from oracle import torch_twin
    rng = np.random.default_rng(d)
    n_ent, n_rel, b = 140, 9, 9
    E, R = (rng.standard_normal((n_ent, d)) * 0.1).astype(np.float32), (rng.standard_normal((n_rel, d)) * 0.1).astype(np.float32)
    m = _lookup_model(E, R, scorer)
    m.train()
    twin = torch_twin.TwinModel(scorer, n_ent, n_rel, d).double()
    with torch.no_grad():
        twin.entity_embedding.weight.copy_(torch.from_numpy(E).double())
        twin.relation_embedding.weight.copy_(torch.from_numpy(R).double())
    ids = lambda lo, hi: torch.from_numpy(rng.integers(lo, hi, (b, 1)).astype(np.int32))       # noqa: E731
    subj, rel_s, rel_o, obj = ids(2, n_ent), ids(2, n_rel), ids(2, n_rel), ids(2, n_ent)
    W1, W2 = torch.from_numpy(rng.standard_normal((b, n_ent - 2))), torch.from_numpy(rng.standard_normal((b, n_ent - 2)))
    own = lambda x1, x2, w1, w2: (torch.tanh(x1) * w1).sum() + (x2 * x2 * w2).sum()       # noqa: E731
    x_sp, x_po = m.sp_prefix_score(subj.cuda(), rel_s.cuda()), m.po_prefix_score(rel_o.cuda(), obj.cuda())
    assert x_sp.requires_grad and x_po.requires_grad and x_sp.shape == (b, n_ent - 2)
    own(x_sp, x_po, W1.float().cuda(), W2.float().cuda()).backward()
    cand = twin.enc_ent(torch.arange(2, n_ent))
    r_sp = twin.score(twin.enc_ent(subj), twin.enc_rel(rel_s), cand, sp=True)
    r_po = twin.score(twin.enc_ent(obj), twin.enc_rel(rel_o), cand, sp=False)
    own(r_sp, r_po, W1, W2).backward()
    np.testing.assert_allclose(x_sp.detach().cpu().numpy(), r_sp.detach().numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(x_po.detach().cpu().numpy(), r_po.detach().numpy(), rtol=0, atol=2e-5)
    for name in ("entity_embedding", "relation_embedding"):
        got, ref = getattr(m, name).weight.grad.cpu().numpy(), getattr(twin, name).weight.grad.numpy()
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-4 * np.abs(ref).max() + 1e-12, err_msg=name)
    with torch.no_grad():
        t = m.triple_score(m.encode_subj(subj.cuda()), m.encode_rel(rel_s.cuda()), m.encode_obj(obj.cuda())).cpu().numpy().reshape(-1)
    want = ko.score_triples(ko.KIND_NAMES[scorer], E[subj.numpy().reshape(-1)].astype(np.float64), R[rel_s.numpy().reshape(-1)].astype(np.float64),
                            E[obj.numpy().reshape(-1)].astype(np.float64))
    np.testing.assert_allclose(t, want, rtol=0, atol=2e-5)
