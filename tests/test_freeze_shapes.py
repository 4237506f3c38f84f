"""OKGE_TRAIN_FREEZE_ENTITIES / OKGE_TRAIN_FREEZE_RELATIONS of okge_train_forward_backward (include/okge.h) through the C ABI, one
case per kernel family and edge: the tile kernels' instantiations without the candidate-gradient product (okge_train64.hip up to
slot size 256, okge_train64k.hip with its stream-K launch above), the wide path without its G^T . Q product (wide_core), and the
prefix backward that forms one table's rows alone (okge_misc.hip).

Per case three calls on the same inputs -- unfrozen, entities frozen, relations frozen:
  * the loss word is bit-equal across the three;
  * where the unfrozen call is order-free (a candidate range or a unique id list, distinct prefix rows with
    OKGE_TRAIN_DISTINCT_PREFIX_ROWS) the trained table's gradient is bit-equal to the unfrozen call's, on cleared buffers and
    accumulating into non-zero ones, and two runs of a frozen call are bit-identical;
  * on an id list with repeats (float atomics: no order to be equal in) the trained table's gradient passes
    lstm_reference.band_check against wide_reference's float64 truth and fp32 yardstick, the rule of test_wide_shapes.py, and two
    runs agree in the loss word, each run's gradient passing that rule on its own (the "-null" entries are the second runs).
    This NARROWS "two runs of each frozen call are bit-identical": with repeated ids the rows of dE / dR are sums of float
    atomicAdds in both the frozen and the unfrozen call, whose order the hardware does not fix, so bit-identity of those
    gradients is not a property either call has;
  * the frozen table's buffer, filled with a NaN pattern, is bitwise untouched, and a NULL pointer in its place is accepted.
The statuses (both flags: -1; either with OKGE_TRAIN_ROW_GRADS: -2) come before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_reference as wr  # noqa: E402
from lstm_reference import band_check  # noqa: E402
from test_wide_shapes import SEED, STEP, dev, make_batch, problem  # noqa: E402

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7FC0BEEF            # a quiet NaN with a payload: any store of a computed value changes the word


@pytest.fixture(scope="module")
def hp():
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    return HotPath("cuda:0")


# scorer, d, n_po, n_sp, N, candidates, loss, smoothing, dropout, OKGE_GT_MBYTES
CASES = [
    ("distmult", 1, 1, 0, 1, "range", "bce", 0.0, None, None),               # smallest shape
    ("complex", 24, 31, 32, 129, "dup", "bce", 0.1, "philox", None),         # label smoothing; repeated ids: atomics
    ("complex", 200, 33, 32, 700, "unique", "kl", 0.0, "philox", None),      # fused_tile64_kernel, the bf16-plane instance
    ("distmult", 256, 0, 65, 129, "range", "bce", 0.0, None, None),          # sp only, two row chunks
    ("distmult", 300, 31, 32, 129, "unique", "bce", 0.0, "philox", None),    # fused_tile64k_kernel, stream-K launch (default)
    ("complex", 512, 65, 0, 700, "range", "kl", 0.0, None, None),            # po only, the largest tile slot size
    ("complex", 528, 31, 32, 129, "dup", "bce", 0.0, "philox", None),        # wide, gathered rows
    ("distmult", 1024, 70, 61, 700, "range", "kl", 0.0, None, 1),            # wide, more than one candidate range
]
IDS = [f"{c[0]}-d{c[1]}-b{c[2]}+{c[3]}-n{c[4]}-{c[5]}-{c[6]}{'-drop' if c[8] else ''}{'-ranges' if c[9] else ''}" for c in CASES]


def setup(case, seed):
    """the case's tables, batch and masks.  Order-free cases: n_rel >= B and distinct prefix ids, none of them a candidate (the
    tables of test_wide_shapes.problem grown by B rows each)"""
    scorer, d, n_po, n_sp, N, mode, loss, smoothing, drop, _ = case
    E, R, z, cand, y = problem(seed, d, n_po, n_sp, N, mode)
    B = n_po + n_sp
    order_free = mode != "dup"
    if order_free:
        rng = np.random.default_rng(seed + 7)
        n_ent = E.shape[0]
        E = np.concatenate([E, (rng.standard_normal((B, d)) * 0.3).astype(np.float32)])
        R = (rng.standard_normal((B + 2, d)) * 0.3).astype(np.float32)
        ent = (n_ent + rng.permutation(B)).astype(np.int32)
        rel = (2 + rng.permutation(B)).astype(np.int32)
        if n_po:
            z["po_obj"], z["po_rel"] = ent[:n_po], rel[:n_po]
        if n_sp:
            z["sp_subj"], z["sp_rel"] = ent[n_po:], rel[n_po:]
    p_ent, p_rel = (0.4, 0.25) if drop else (0.0, 0.0)
    masks = wr.philox_masks(SEED, STEP, n_po, n_sp, N, d, p_ent, p_rel) if drop else None
    batch = make_batch(z, cand, mode, y, drop, p_ent, p_rel, masks)
    return E, R, z, cand, y, batch, masks, (p_ent, p_rel), order_free


def nan_like(a):
    return torch.full(a.shape, NAN_BITS, dtype=torch.int32, device="cuda:0").view(torch.float32)


def untouched(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64).numpy()


def call(hp, E, R, case, batch, dE, dR, freeze=None, grads_zero=True, distinct=False):
    loss = hp.forward_backward(E, R, case[0], batch, dE, dR, loss=case[6], label_smoothing=case[7], grads_zero=grads_zero,
                               distinct_prefix_rows=distinct, freeze=freeze)
    torch.cuda.synchronize()
    return bits(loss)[0]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_frozen_calls_against_the_unfrozen_call(hp, case, monkeypatch):
    monkeypatch.delenv("OKGE_GT_MBYTES", raising=False)
    if case[9] is not None:
        monkeypatch.setenv("OKGE_GT_MBYTES", str(case[9]))
        assert wr.plan(case[2] + case[3], case[4], case[1], case[9])["n_ranges"] > 1
    scorer, d, n_po, n_sp, N, mode, loss, smoothing, drop, _ = case
    E, R, z, cand, y, batch, masks, (p_ent, p_rel), order_free = setup(case, 500 + CASES.index(case))
    Et, Rt = dev(E), dev(R)
    zE, zR = torch.zeros_like(Et), torch.zeros_like(Rt)
    # ---- cleared buffers -------------------------------------------------------------------------------------------------
    dE_u, dR_u = zE.clone(), zR.clone()
    loss_u = call(hp, Et, Rt, case, batch, dE_u, dR_u, None, True, order_free)
    dE_fe, dR_fe = nan_like(Et), zR.clone()
    loss_fe = call(hp, Et, Rt, case, batch, dE_fe, dR_fe, "entities", True, order_free)
    dE_fr, dR_fr = zE.clone(), nan_like(Rt)
    loss_fr = call(hp, Et, Rt, case, batch, dE_fr, dR_fr, "relations", True, order_free)
    assert loss_u == loss_fe == loss_fr, (loss_u, loss_fe, loss_fr)
    assert untouched(dE_fe) and untouched(dR_fr)                            # candidate rows and prefix rows alike
    # ---- a NULL pointer for the frozen buffer (hotpath raises on any status but 0); also the second run of each frozen call ---
    dR_fe2, dE_fr2 = zR.clone(), zE.clone()
    assert call(hp, Et, Rt, case, batch, None, dR_fe2, "entities", True, order_free) == loss_u
    assert call(hp, Et, Rt, case, batch, dE_fr2, None, "relations", True, order_free) == loss_u
    if order_free:
        assert np.array_equal(bits(dR_fe), bits(dR_u)) and np.array_equal(bits(dE_fr), bits(dE_u))
        assert np.array_equal(bits(dR_fe2), bits(dR_fe)) and np.array_equal(bits(dE_fr2), bits(dE_fr))
        # ---- accumulating into non-zero buffers -------------------------------------------------------------------------------
        rng = np.random.default_rng(9)
        dE0, dR0 = (rng.standard_normal(E.shape) * 1e-4).astype(np.float32), (rng.standard_normal(R.shape) * 1e-4).astype(np.float32)
        aE_u, aR_u = dev(dE0), dev(dR0)
        assert call(hp, Et, Rt, case, batch, aE_u, aR_u, None, False, True) == loss_u
        aE_fe, aR_fe = nan_like(Et), dev(dR0)
        assert call(hp, Et, Rt, case, batch, aE_fe, aR_fe, "entities", False, True) == loss_u
        aE_fr, aR_fr = dev(dE0), nan_like(Rt)
        assert call(hp, Et, Rt, case, batch, aE_fr, aR_fr, "relations", False, True) == loss_u
        assert untouched(aE_fe) and untouched(aR_fr)
        assert np.array_equal(bits(aR_fe), bits(aR_u)) and np.array_equal(bits(aE_fr), bits(aE_u))
    else:
        t = wr.truth(scorer, E, R, z, cand, y, loss, smoothing, p_ent, p_rel, masks)
        yd = wr.yardstick(scorer, E, R, z, cand, y, loss, smoothing, p_ent, p_rel, masks)
        tag = IDS[CASES.index(case)]
        worst = {}
        for name, got, key in (("unfrozen:dE", dE_u, "dE"), ("unfrozen:dR", dR_u, "dR"), ("freeze_entities:dR", dR_fe, "dR"),
                               ("freeze_entities-null:dR", dR_fe2, "dR"), ("freeze_relations:dE", dE_fr, "dE"),
                               ("freeze_relations-null:dE", dE_fr2, "dE")):
            worst[name] = band_check(f"{tag}:{name}", got, t[key], yd[key])
        print(f"freeze-bands {tag} " + " ".join(f"{k}=max{w[0]:.2f}/rms{w[1]:.2f}" for k, w in worst.items()))
        want = t["loss"]
        got = np.array([loss_u], np.int64).view(np.float64)[0]
        assert abs(got - want) <= 3e-5 * abs(want)


def _raw(hp, okge_lib, flags, dE, dR, loss, d=24):
    E, R, z, cand, y = problem(91, d, 3, 2, 30, "range")
    b = make_batch(z, cand, "range", y)
    pb, c, keep = hp._batch(b)
    t = hp._tables(dev(E), dev(R), "complex")
    pos, keep_pos = hp._positives(b)
    ws = hp.workspace(5, 30, d)
    rc = okge_lib.okge_train_forward_backward(ctypes.byref(t), ctypes.byref(pb), ctypes.byref(c), ctypes.byref(pos), 0, 0.0, 150.0, flags,
                                              loss.data_ptr(), None if dE is None else dE.data_ptr(), None if dR is None else dR.data_ptr(),
                                              None, 0, ws.data_ptr(), hp._ws_bytes, hp._stream())
    torch.cuda.synchronize()
    return rc, (E.shape, R.shape)


def test_statuses_before_any_launch(hp, okge_lib):
    from open_knowledge_graph_embeddings_amd import _native as N_
    FE, FR = N_.OKGE_TRAIN_FREEZE_ENTITIES, N_.OKGE_TRAIN_FREEZE_RELATIONS
    assert (FE, FR) == (64, 128)
    for d in (24, 520):                                                       # the tile kernels' route and the wide one
        shapes = _raw(hp, okge_lib, N_.OKGE_TRAIN_LOSS_ONLY, None, None, torch.zeros(1, dtype=torch.float64, device="cuda:0"), d)[1]
        for flags, code, text in ((FE | FR, -1, b"nothing to train"), (FE | N_.OKGE_TRAIN_ROW_GRADS, -2, b"dense call"),
                                  (FR | N_.OKGE_TRAIN_ROW_GRADS, -2, b"dense call")):
            dE, dR = nan_like(torch.empty(shapes[0])), nan_like(torch.empty(shapes[1]))
            loss = torch.full((1,), NAN_BITS, dtype=torch.int64, device="cuda:0").view(torch.float64)
            rc, _ = _raw(hp, okge_lib, flags | N_.OKGE_TRAIN_GRADS_ZERO, dE, dR, loss, d)
            assert rc == code, (d, flags, rc)
            assert text in okge_lib.okge_last_error(), okge_lib.okge_last_error()
            assert untouched(dE) and untouched(dR) and int(loss.view(torch.int64)[0]) == NAN_BITS
    # with OKGE_TRAIN_LOSS_ONLY the flags change nothing: the loss word of the plain loss-only call, no buffer looked at
    out = []
    for flags in (0, FE, FR):
        loss = torch.zeros(1, dtype=torch.float64, device="cuda:0")
        rc, _ = _raw(hp, okge_lib, flags | N_.OKGE_TRAIN_LOSS_ONLY, None, None, loss)
        assert rc == 0
        out.append(bits(loss)[0])
    assert out[0] == out[1] == out[2]
