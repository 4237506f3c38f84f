"""NumPy restatement of the top-k order of include/okge.h ("top-k link prediction"), tests only.

  * candidate a precedes b if score(a) > score(b);
  * equal scores (float comparison: -0.0 == +0.0) -> the smaller candidate column first;
  * a NaN orders as -inf (after every number, before the padding) and is reported as it is;
  * filtered columns are dropped outright;
  * a row with fewer than k eligible candidates is padded with score = -inf, col = -1, id = -1.
Implemented as a stable lexsort on (col, -score) after mapping NaN to -inf.
"""
import numpy as np


def _order(scores, cols):
    key = np.where(np.isnan(scores), -np.inf, scores).astype(np.float32)
    return np.lexsort((cols, -key))                       # primary: -score ascending, secondary: column ascending


def _pad(scores, cols, k):
    s = np.full(k, -np.inf, np.float32)
    c = np.full(k, -1, np.int32)
    n = min(k, len(cols))
    s[:n], c[:n] = scores[:n], cols[:n]
    return s, c


def topk_rows(scores, k, filt_ptr=None, filt_col=None, col0=0, ids=None, first_id=None):
    """scores (B, N) fp32 of the candidate columns col0 .. col0 + N - 1; filter columns are global.
    -> (scores (B, k) fp32, cols (B, k) int32 global, ids (B, k) int32: ids[col - col0] or first_id + col - col0, -1 padded)"""
    scores = np.asarray(scores, np.float32)
    B, N = scores.shape
    out_s, out_c = np.empty((B, k), np.float32), np.empty((B, k), np.int32)
    cols = np.arange(N, dtype=np.int64) + col0
    for b in range(B):
        keep = np.ones(N, bool)
        if filt_ptr is not None:
            f = np.asarray(filt_col[int(filt_ptr[b]):int(filt_ptr[b + 1])], np.int64) - col0
            keep[f[(f >= 0) & (f < N)]] = False
        s, c = scores[b][keep], cols[keep]
        o = _order(s, c)
        out_s[b], out_c[b] = _pad(s[o], c[o], k)
    return out_s, out_c, ids_of(out_c, col0, ids, first_id)


def ids_of(cols, col0=0, ids=None, first_id=None):
    loc = np.maximum(cols - col0, 0)
    if ids is not None:
        e = np.asarray(ids, np.int32)[loc]
    else:
        e = (loc + (0 if first_id is None else first_id)).astype(np.int32)
    return np.where(cols >= 0, e, -1).astype(np.int32)


def merge_lists(scores, cols, k=None):
    """(L, B, k') lists (padding: col = -1) -> the (B, k) list of their union under the same rule"""
    scores, cols = np.asarray(scores, np.float32), np.asarray(cols, np.int32)
    L, B, kq = scores.shape
    k = kq if k is None else k
    out_s, out_c = np.empty((B, k), np.float32), np.empty((B, k), np.int32)
    for b in range(B):
        s, c = scores[:, b].reshape(-1), cols[:, b].reshape(-1)
        live = c >= 0
        s, c = s[live], c[live]
        o = _order(s, c)
        out_s[b], out_c[b] = _pad(s[o], c[o], k)
    return out_s, out_c


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def assert_same(got, want, what=""):
    """scores bit-equal (a NaN is a NaN, -0.0 is not +0.0), columns / ids identical"""
    gs, ws = np.asarray(got[0]), np.asarray(want[0])
    assert gs.shape == ws.shape, (what, gs.shape, ws.shape)
    bad = np.argwhere(bits(gs) != bits(ws))
    assert len(bad) == 0, (what, "scores differ at", bad[:5].tolist(), gs[tuple(bad[0])], ws[tuple(bad[0])])
    for i, (g, w) in enumerate(zip(got[1:], want[1:])):
        g, w = np.asarray(g), np.asarray(w)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, f"index array {i} differs at", bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
