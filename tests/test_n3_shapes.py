"""okge_n3_forward_backward (csrc/okge_n3.hip) at its edge shapes against the float64 restatement of tests/n3_reference.py:
slot sizes with and without 16-byte rows (2, 6: single floats; 12, 200, 516, 4096: float4), one row and more rows than a
workgroup takes, a candidate range and id lists that repeat ids, 0 / 1 / 2 candidate passes, Philox masks and explicit masks,
dense tables, occurrence rows, and the flags that turn the float atomics off.

Bounds.  A gradient element is x |x| ks with x = fl(e s): three fp32 roundings, a fourth when it is added to a zero (exact) or
to a sum of like-signed terms -- every term of one element has the sign of e -- so 1e-6 relative per element holds up to about
a dozen occurrences of one id; the tables below keep an id under that.  Into a buffer that already holds a gradient:
|got - (before + want)| <= 2^-23 (|before| + |want|) + 1e-6 |want|, which leaves room for TWO roundings against the held value;
the accumulation cases therefore name every element at most twice (once as a candidate, once as a prefix row).  The value is a
double sum of cubes of fp32 x: 1e-6 relative."""
import ctypes

import numpy as np
import pytest
import torch

import n3_reference as nr
from oracle import kge_oracle as ko

pytestmark = pytest.mark.gpu
SEED, STEP = 0xBEEF00051, 9
GUARD = 64                                  # elements of sentinel on either side of every buffer (keeps 16-byte alignment)
LOSS_ONLY, UNIQUE, DISTINCT, ROW_GRADS = 2, 4, 8, 32


@pytest.fixture(scope="module")
def hp():
    from open_knowledge_graph_embeddings_amd.hotpath import HotPath
    return HotPath("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def problem(seed, d, n_po, n_sp, N, mode, distinct=False, twice=False):
    """mode: 'range' (ids first .. first + N - 1, first = 3), 'dup' (a list that repeats ids), 'unique' (distinct ids, any order).
    distinct: every prefix id once and no prefix entity a candidate.  twice: no element is named more than twice (prefix ids
    distinct among themselves, a 'dup' list repeats an id at most twice and shares none with the prefixes)."""
    rng = np.random.default_rng(seed)
    B, first = n_po + n_sp, 3
    n_pool = {"range": N, "dup": max(2, (N + 1) // 2), "unique": N + 5}[mode]          # entity rows the candidates draw from
    n_ent, n_rel = first + n_pool + B + 2, max(7, (B if (distinct or twice) else B // 3) + 3)
    E, R = rng.standard_normal((n_ent, d)).astype(np.float32) * 0.7, rng.standard_normal((n_rel, d)).astype(np.float32) * 0.7
    for T in (E, R):                                    # exact zeros of both signs, a row of negative entries
        T[rng.random(T.shape) < 0.05] = 0.0
        T[rng.random(T.shape) < 0.02] = -0.0
        T[2] = -np.abs(T[2])
    pool = np.arange(first, first + n_pool)
    if mode == "range":
        cand = pool
    elif mode == "unique":
        cand = rng.permutation(pool)[:N]
    elif twice:
        cand = rng.permutation(np.concatenate([pool, pool]))[:N]
    else:
        cand = rng.integers(first, first + n_pool, N)
        cand[-1] = cand[0]
    outside = np.arange(first + n_pool, n_ent)           # entity rows no candidate names
    if distinct or (twice and mode == "dup"):
        ent = rng.permutation(outside)[:B]
    elif twice:
        ent = rng.permutation(np.arange(2, n_ent))[:B]
    else:
        ent = rng.integers(2, n_ent, B)
    rel = rng.permutation(np.arange(2, n_rel))[:B] if (distinct or twice) else rng.integers(2, n_rel, B)
    ent, rel = ent.astype(np.int32), rel.astype(np.int32)
    z = dict(E=E, R=R, cand=cand.astype(np.int32), mode=mode, first=first, N=N, n_po=n_po, n_sp=n_sp, d=d)
    z["po"] = (rel[:n_po], ent[:n_po]) if n_po else None
    z["sp"] = (ent[n_po:], rel[n_po:]) if n_sp else None
    return z


def masks_for(hp, z, drop, p_ent, p_rel, seed):
    """the five keep masks: drawn here ('keep'), or read off the library's own encode on the same spec ('philox'), which is the
    gather the tile kernels' masks are pinned to; checked against the oracle's Philox as well"""
    from open_knowledge_graph_embeddings_amd import hotpath as H
    if drop is None:
        return {}, {}
    rng = np.random.default_rng(seed)
    rows = dict(keep_cand=(z["N"], H.STREAM_CAND, p_ent), keep_po_ent=(z["n_po"], H.STREAM_PO_ENT, p_ent),
                keep_po_rel=(z["n_po"], H.STREAM_PO_REL, p_rel), keep_sp_ent=(z["n_sp"], H.STREAM_SP_ENT, p_ent),
                keep_sp_rel=(z["n_sp"], H.STREAM_SP_REL, p_rel))
    masks, specs = {}, {}
    for key, (n, stream, p) in rows.items():
        if n == 0 or p <= 0:
            continue
        if drop == "keep":
            masks[key] = rng.random((n, z["d"])) >= p
            specs[key] = H.DropoutSpec(p=p, keep=dev(masks[key].astype(np.uint8)))
        else:
            specs[key] = H.DropoutSpec(p, SEED, stream, STEP)
            ones = torch.ones((n, z["d"]), device="cuda:0")
            masks[key] = hp.encode_rows(ones, None, 0, n, specs[key]).cpu().numpy() > 0
            assert np.array_equal(masks[key], ko.dropout_keep_mask(SEED, stream, STEP, n, z["d"], p)), key
    return masks, specs


def make_batch(z, specs):
    from open_knowledge_graph_embeddings_amd import hotpath as H
    b = H.PrefixBatch()
    if z["po"] is not None:
        b.po_rel, b.po_obj = dev(z["po"][0]), dev(z["po"][1])
    if z["sp"] is not None:
        b.sp_subj, b.sp_rel = dev(z["sp"][0]), dev(z["sp"][1])
    if z["mode"] == "range":
        b.cand_first, b.n_cand = z["first"], z["N"]
    else:
        b.cand_ids, b.n_cand = dev(z["cand"]), z["N"]
    for key, spec in specs.items():
        setattr(b, "drop_" + key[5:], spec)
    return b


def guarded(n, dtype, fill):
    """a buffer of n elements between two sentinels of GUARD elements -> (whole block, the buffer)"""
    raw = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
    return raw, raw[GUARD:GUARD + n]


def guards_intact(raw, n, fill):
    lo, hi = raw[:GUARD], raw[GUARD + n:]
    if isinstance(fill, float) and fill != fill:
        return bool(torch.isnan(lo).all() and torch.isnan(hi).all())
    return bool((lo == fill).all() and (hi == fill).all())


class Call:
    """one okge_n3_forward_backward problem with every buffer between sentinels and the workspace at its exact size"""

    def __init__(self, hp, lib, z, batch, scorer, row_grads=False):
        self.hp, self.lib, self.z, self.batch = hp, lib, z, batch
        self.pb, self.c, self.keep = hp._batch(batch)
        self.E, self.R = dev(z["E"]), dev(z["R"])
        self.t = hp._tables(self.E, self.R, scorer)
        B, N, d = z["n_po"] + z["n_sp"], z["N"], z["d"]
        self.shape_e = (N + B, d) if row_grads else z["E"].shape
        self.shape_r = (B, d) if row_grads else z["R"].shape
        self.need = int(lib.okge_n3_workspace_bytes(B, N, d))
        assert self.need > 0 and self.need % 256 == 0

    def run(self, coef, passes, normalizer, flags, before=None, ws_bytes=None, grads=True):
        ne, nr_ = int(np.prod(self.shape_e)), int(np.prod(self.shape_r))
        nan = float("nan")
        raw_e, gE = guarded(ne, torch.float32, nan)
        raw_r, gR = guarded(nr_, torch.float32, nan)
        raw_v, reg = guarded(1, torch.float64, nan)
        raw_w, ws = guarded(self.need, torch.uint8, 0xA5)
        if grads:
            gE.copy_(dev(before[0].reshape(-1))) if before is not None else gE.zero_()
            gR.copy_(dev(before[1].reshape(-1))) if before is not None else gR.zero_()
        rc = self.lib.okge_n3_forward_backward(ctypes.byref(self.t), ctypes.byref(self.pb), ctypes.byref(self.c), float(coef), int(passes),
                                               float(normalizer), int(flags), reg.data_ptr(), gE.data_ptr(), gR.data_ptr(), ws.data_ptr(),
                                               self.need if ws_bytes is None else ws_bytes, self.hp._stream())
        torch.cuda.synchronize()
        assert guards_intact(raw_e, ne, nan) and guards_intact(raw_r, nr_, nan) and guards_intact(raw_v, 1, nan)
        assert guards_intact(raw_w, self.need, 0xA5)
        return rc, reg.cpu().numpy()[0], gE.cpu().numpy().reshape(self.shape_e), gR.cpu().numpy().reshape(self.shape_r)


def reference(z, masks, coef, passes, normalizer, p_ent, p_rel):
    return nr.n3_term(z["E"], z["R"], z["po"], z["sp"], z["cand"], coef, passes, normalizer, p_ent=p_ent, p_rel=p_rel, **masks)


def close_rel(got, want, tag):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(np.abs(want), 1e-300)).max()) if want.size else 0.0
    print(f"{tag}: worst relative error {worst:.3e}")
    assert np.all(err <= 1e-6 * np.abs(want)), (tag, worst)


#         d, n_po, n_sp, N, mode, passes, drop, flags, scorer
CASES = [(2, 1, 0, 1, "range", 1, None, 0, "complex"),
         (6, 0, 1, 63, "range", 2, "keep", 0, "distmult"),
         (12, 3, 2, 130, "dup", 1, "philox", 0, "complex"),
         (200, 65, 64, 130, "range", 2, "philox", 0, "complex"),
         (516, 3, 2, 63, "dup", 1, "keep", 0, "distmult"),
         (4096, 3, 2, 130, "range", 1, "philox", 0, "complex"),
         (4096, 65, 64, 63, "dup", 2, None, 0, "distmult"),
         (6, 3, 2, 130, "range", 0, "philox", 0, "complex"),
         (200, 1, 0, 1, "dup", 1, "keep", 0, "complex"),
         (12, 65, 64, 63, "unique", 1, "philox", UNIQUE, "distmult"),
         (200, 3, 2, 63, "dup", 1, "philox", ROW_GRADS, "complex"),
         (6, 65, 64, 130, "range", 2, "keep", ROW_GRADS, "distmult"),
         (516, 3, 2, 130, "range", 1, "philox", DISTINCT, "complex"),
         (2, 0, 1, 63, "unique", 2, "keep", UNIQUE | DISTINCT, "distmult")]


@pytest.mark.parametrize("case", CASES, ids=[f"d{c[0]}-b{c[1]}+{c[2]}-n{c[3]}-{c[4]}-x{c[5]}-{c[6]}-f{c[7]}" for c in CASES])
def test_value_and_gradient_against_float64(hp, okge_lib, case):
    d, n_po, n_sp, N, mode, passes, drop, flags, scorer = case
    p_ent, p_rel = (0.35, 0.2) if drop else (0.0, 0.0)
    z = problem(1000 + d + N + n_po, d, n_po, n_sp, N, mode, distinct=bool(flags & DISTINCT))
    masks, specs = masks_for(hp, z, drop, p_ent, p_rel, seed=d)
    coef, normalizer = nr.coef(0.013, 0.2), float((n_po + n_sp) * N)
    row_grads = bool(flags & ROW_GRADS)
    want = reference(z, masks, coef, passes, normalizer, p_ent, p_rel)
    wE, wR = (want["gE"], want["gR"]) if row_grads else (want["dE"], want["dR"])
    call = Call(hp, okge_lib, z, make_batch(z, specs), scorer, row_grads)
    rc, value, gE, gR = call.run(coef, passes, normalizer, flags)
    assert rc == 0, okge_lib.okge_last_error()
    assert abs(value - want["value"]) <= 1e-6 * abs(want["value"]), (value, want["value"])
    assert np.abs(wE).max() > 0 and np.abs(wR).max() > 0
    close_rel(gE, wE, "dE")
    close_rel(gR, wR, "dR")
    if not row_grads:
        assert not gE[:2].any()                       # rows in front of the candidates (row 2: a prefix id may name it)
    # a second run: the value bit for bit, the gradients wherever no float atomic ran
    rc2, value2, gE2, gR2 = call.run(coef, passes, normalizer, flags)
    assert rc2 == 0 and value2 == value
    cand_atomic = mode == "dup" and not row_grads
    prefix_atomic = not row_grads and not (flags & DISTINCT)
    if not prefix_atomic:
        assert np.array_equal(gR2, gR)
    quiet = np.ones(gE.shape[0], bool)
    if cand_atomic:
        quiet[z["cand"]] = False
    if prefix_atomic:
        for pair, at in ((z["po"], 1), (z["sp"], 0)):
            if pair is not None:
                quiet[pair[at]] = False
    assert np.array_equal(gE2[quiet], gE[quiet])
    # value only: not one gradient byte is touched
    rc3, value3, nE, nR = call.run(coef, passes, normalizer, (flags & ~ROW_GRADS) | LOSS_ONLY, grads=False)
    assert rc3 == 0 and value3 == value and np.isnan(nE).all() and np.isnan(nR).all()


ACC = [(12, 3, 2, 130, "range", 1, "philox", 0), (6, 65, 64, 130, "range", 2, "keep", 0), (200, 3, 2, 63, "dup", 1, "philox", 0),
       (516, 65, 64, 63, "unique", 2, None, UNIQUE), (4096, 3, 2, 63, "range", 1, "keep", ROW_GRADS), (2, 3, 2, 63, "dup", 1, None, ROW_GRADS),
       (200, 65, 64, 130, "range", 1, "philox", DISTINCT)]


@pytest.mark.parametrize("case", ACC, ids=[f"d{c[0]}-b{c[1]}+{c[2]}-n{c[3]}-{c[4]}-x{c[5]}-{c[6]}-f{c[7]}" for c in ACC])
def test_gradient_adds_to_what_the_buffers_hold(hp, okge_lib, case):
    d, n_po, n_sp, N, mode, passes, drop, flags = case
    p_ent, p_rel = (0.3, 0.25) if drop else (0.0, 0.0)
    z = problem(2000 + d + N, d, n_po, n_sp, N, mode, distinct=bool(flags & DISTINCT), twice=True)
    masks, specs = masks_for(hp, z, drop, p_ent, p_rel, seed=d + 1)
    coef, normalizer = 0.02, 37.0
    row_grads = bool(flags & ROW_GRADS)
    want = reference(z, masks, coef, passes, normalizer, p_ent, p_rel)
    wE, wR = (want["gE"], want["gR"]) if row_grads else (want["dE"], want["dR"])
    call = Call(hp, okge_lib, z, make_batch(z, specs), "distmult", row_grads)
    rng = np.random.default_rng(d)
    before = [(rng.standard_normal(s) * m).astype(np.float32) for s, m in ((call.shape_e, np.abs(wE).max()), (call.shape_r, np.abs(wR).max()))]
    rc, _, gE, gR = call.run(coef, passes, normalizer, flags, before=before)
    assert rc == 0, okge_lib.okge_last_error()
    for got, b, w, tag in ((gE, before[0], wE, "dE"), (gR, before[1], wR, "dR")):
        b = b.astype(np.float64)
        err, tol = np.abs(got - (b + w)), 2.0 ** -23 * (np.abs(b) + np.abs(w)) + 1e-6 * np.abs(w)
        print(f"{tag}: worst error / bound {float((err / np.maximum(tol, 1e-300)).max()):.3f}")
        assert np.all(err <= tol), tag
        assert np.array_equal(got[w == 0], b[w == 0].astype(np.float32))            # what the term does not name keeps its bits


def test_workspace_is_exact_and_refusals_come_before_any_launch(hp, okge_lib):
    z = problem(5, 12, 3, 2, 63, "range")
    call = Call(hp, okge_lib, z, make_batch(z, {}), "complex")
    nan_e = np.full(z["E"].shape, np.nan, np.float32), np.full(z["R"].shape, np.nan, np.float32)

    def refused(rc_want, **kw):
        args = dict(coef=0.01, passes=1, normalizer=10.0, flags=0, before=nan_e)
        args.update(kw)
        rc, value, gE, gR = call.run(**args)
        assert rc == rc_want, (rc, okge_lib.okge_last_error())
        assert np.isnan(value) and np.isnan(gE).all() and np.isnan(gR).all()          # nothing ran

    refused(-3, ws_bytes=call.need - 1)
    refused(-1, passes=3)
    refused(-1, passes=-1)
    refused(-1, normalizer=0.0)
    for scorer in (2, 3):                                                             # the data-bias scorers
        call.t.scorer = scorer
        refused(-2)
        assert b"okge_n3_forward_backward" in okge_lib.okge_last_error()
    call.t.scorer = 0
    call.c.table, call.c.table_rows = call.E.data_ptr(), z["E"].shape[0]              # candidates from a caller's table
    refused(-1)
    call.c.table, call.c.table_rows = None, 0
    call.t.d = 4098                                                                   # (only the descriptor: refused before any use)
    refused(-2)
    assert okge_lib.okge_n3_workspace_bytes(5, 63, 4098) == 0 and okge_lib.okge_n3_workspace_bytes(0, 63, 12) == 0
    call.t.d = 12
    rc, value, gE, gR = call.run(0.01, 1, 10.0, 0)
    assert rc == 0 and np.isfinite(value) and np.isfinite(gE).all()
