"""A plain numpy / torch-CPU restatement of the score backward (okge_prefix_score_backward, csrc/okge_gemm.hip) and of the two
row kernels around it (okge_encode_rows, csrc/okge_misc.hip; okge_scatter_rows, csrc/okge_gemm.hip) at a chosen dtype.  Not a
conftest: the tests import it.

  q = fold(ent, rel)          sp: [e1 r1 - e2 r2, e2 r1 + e1 r2]   po: [e1 r1 + e2 r2, e2 r1 - e1 r2]   DistMult: e * r
  dC = G^T . q                dQ = G . C  ->  (d_ent, d_rel) by the transpose of the fold
  encode_rows                 table[id] * (keep ? fp32(1) / (fp32(1) - fp32(p)) : 0)
  scatter_rows                positions stably sorted by id, the rows of a run of equal ids summed in that order from 0, the sum
                              added to the table's row; row 0 (padding_idx) receives nothing

float64 is the truth.  float32 is the CALIBRATION YARDSTICK, and restates the kernels' arithmetic, not a library matmul: the
fold with every product rounded on its own (fold_complex), every matrix product ONE sequential fp32 accumulate over its
contraction (an fp32 MFMA accumulation is a k-ordered chain; tests/test_dq_split.fp32_chain, vectorised over the output block),
G . C cut into the split ranges launch_score_backward uses (split_plan restates that cut: the library does not export it) with
the slabs added in split order from 0, G^T . q one chain over b, the fold backward in plain fp32."""
import numpy as np
import torch

GM, GN, GK, MAX_SPLITS = 64, 64, 16, 64                # gemm_f32_kernel's tile and the cap on its split count
U = 2.0 ** -24                                         # fp32 unit roundoff

torch.set_num_threads(max(1, min(16, torch.get_num_threads())))      # the GPU box gives a test 16 CPUs


def split_plan(b, n, d):
    """(splits, k_per) of dQ = G . C as launch_score_backward cuts the n candidates: as many splits as the 64-candidate
    quarters allow, at most 64 and at most 1024 workgroups in all; k_per rounded up to whole 16-chunks, which can leave
    fewer splits than asked; split s covers candidates [s k_per, min(n, (s + 1) k_per))"""
    tiles = ((b + GM - 1) // GM) * ((d + GN - 1) // GN)
    splits = max(1, min(MAX_SPLITS, 1024 // max(tiles, 1), (n + 4 * GK - 1) // (4 * GK)))
    k_per = ((n + splits - 1) // splits + GK - 1) // GK * GK
    return (n + k_per - 1) // k_per, k_per


def workspace_floats(b, d):
    """what the call may touch of its workspace: q, dq and at most 64 slabs, each [b][d]"""
    return (2 + MAX_SPLITS) * b * d


def _np(x, dtype):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=dtype)


def fold(scorer, sp, ent, rel, dtype=np.float64):
    """the query rows; at float32 every product and every sum is rounded on its own, as fold_complex / __fmul_rn do"""
    e, r = _np(ent, dtype), _np(rel, dtype)
    if scorer == "distmult":
        return e * r
    h = e.shape[1] // 2
    e1, e2, r1, r2 = e[:, :h], e[:, h:], r[:, :h], r[:, h:]
    a, b, c, dd = e1 * r1, e2 * r2, e2 * r1, e1 * r2
    return np.concatenate([a - b, c + dd] if sp else [a + b, c - dd], axis=1)


def fold_backward(scorer, sp, ent, rel, dq, dtype=np.float64):
    """(d_ent, d_rel): the transpose of the fold applied to dq"""
    e, r, g = _np(ent, dtype), _np(rel, dtype), _np(dq, dtype)
    if scorer == "distmult":
        return g * r, g * e
    h = e.shape[1] // 2
    e1, e2, r1, r2, g1, g2 = e[:, :h], e[:, h:], r[:, :h], r[:, h:], g[:, :h], g[:, h:]
    if sp:
        return (np.concatenate([g1 * r1 + g2 * r2, g2 * r1 - g1 * r2], axis=1),
                np.concatenate([g1 * e1 + g2 * e2, g2 * e1 - g1 * e2], axis=1))
    return (np.concatenate([g1 * r1 - g2 * r2, g1 * r2 + g2 * r1], axis=1),
            np.concatenate([g1 * e1 + g2 * e2, g1 * e2 - g2 * e1], axis=1))


def chain(A, B, transpose_a=False):
    """A . B (A^T . B with transpose_a) as ONE sequential fp32 fma chain over the contraction for every output element:
    acc = fp32(acc + a_k b_k), k ascending, from 0.  The product of two fp32 numbers is exact in float64 and the sum is rounded
    to float64 and then to fp32 -- an fma but for the rare double rounding.  fp32 numpy in, fp32 numpy out."""
    A64, B64 = torch.from_numpy(_np(A, np.float64)), torch.from_numpy(_np(B, np.float64))
    if not transpose_a:
        A64 = A64.t().contiguous()                     # [K][M]: a step reads one row of each operand
    K, M = A64.shape
    acc = torch.zeros((M, B64.shape[1]), dtype=torch.float64)
    acc32 = torch.zeros((M, B64.shape[1]), dtype=torch.float32)
    for k in range(K):
        acc.addcmul_(A64[k][:, None], B64[k][None, :])
        acc32.copy_(acc)
        acc.copy_(acc32)
    return acc32.numpy()


def product_dq(G, C, dtype=np.float64):
    """dQ = G . C.  float32: the chain per split range of split_plan, the slabs added in split order from 0 (one slab: no add)"""
    if dtype == np.float64:
        return _np(G, np.float64) @ _np(C, np.float64)
    G, C = _np(G, np.float32), _np(C, np.float32)
    b, n = G.shape
    splits, k_per = split_plan(b, n, C.shape[1])
    if splits == 1:
        return chain(G, C)
    out = np.zeros((b, C.shape[1]), np.float32)
    for s in range(splits):
        out = out + chain(G[:, s * k_per:min(n, (s + 1) * k_per)], C[s * k_per:min(n, (s + 1) * k_per)])
    return out


def product_dc(G, Q, dtype=np.float64):
    """dC = G^T . Q.  float32: one chain over the b rows"""
    if dtype == np.float64:
        return _np(G, np.float64).T @ _np(Q, np.float64)
    return chain(_np(G, np.float32), _np(Q, np.float32), transpose_a=True)


def score_backward(scorer, sp, G, ent, rel, cand, dtype=np.float64, matmul=None):
    """dict q, dq, d_ent, d_rel, d_cand at dtype from fp32 inputs.  matmul (float32 only): a function (A, B) -> A . B that
    replaces the chains, for the record beside them (torch's blocked CPU matmul)"""
    q = fold(scorer, sp, ent, rel, dtype)
    if matmul is None:
        dq, dc = product_dq(G, cand, dtype=dtype), product_dc(G, q, dtype)
    else:
        dq, dc = matmul(_np(G, dtype), _np(cand, dtype)), matmul(np.ascontiguousarray(_np(G, dtype).T), q)
    d_ent, d_rel = fold_backward(scorer, sp, ent, rel, dq, dtype)
    return dict(q=q, dq=dq, d_ent=d_ent, d_rel=d_rel, d_cand=dc)


def torch_matmul32(A, B):
    return (torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)) @ torch.from_numpy(np.ascontiguousarray(B, dtype=np.float32))).numpy()


def abs_product_dq(G, C):
    """sum_n |g| |c| in float64: the scale of the classical bound of dQ"""
    return np.abs(_np(G, np.float64)) @ np.abs(_np(C, np.float64))


def abs_product_dc(G, Q):
    return np.abs(_np(G, np.float64)).T @ np.abs(_np(Q, np.float64))


# ---- the row kernels ---------------------------------------------------------------------------------------------------
def drop_mult(keep, p, dtype=np.float32):
    """the multiplier of every element: keep ? fp32(1) / (fp32(1) - fp32(p)) : 0 (the library's fp32 scale), at dtype"""
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(np.asarray(keep, dtype=bool), scale, np.float32(0.0)).astype(dtype)


def row_ids(ids, first_id, n):
    return np.arange(first_id, first_id + n, dtype=np.int64) if ids is None else _np(ids, np.int64).reshape(-1)[:n]


def encode_rows(table, ids=None, first_id=0, n=None, mult=None, dtype=np.float32):
    """table[id] * mult (mult [n][d] from drop_mult, None: no dropout)"""
    t = _np(table, dtype)
    rows = t[row_ids(ids, first_id, len(ids) if ids is not None else n)]
    return rows if mult is None else rows * np.asarray(mult, dtype=dtype)


def scatter_rows(rows, ids, first_id, table_grad, mult=None, dtype=np.float32):
    """-> (table_grad + per-row sums, sum |row mult| per table row, longest-run length per table row).  The positions are
    sorted by id (stable); the rows of a run are added one after the other, in that order, to an accumulator that starts at 0,
    every product row * mult rounded on its own; the accumulator is added to the table's row.  Row 0 receives nothing."""
    r = _np(rows, dtype)
    if mult is not None:
        r = r * np.asarray(mult, dtype=dtype)
    out = _np(table_grad, dtype).copy()
    n = r.shape[0]
    mag, run = np.zeros(out.shape, np.float64), np.zeros(out.shape[0], np.int64)
    if n == 0:
        return out, mag, run
    id_ = row_ids(ids, first_id, n)
    order = np.argsort(id_, kind="stable")
    sid = id_[order]
    start = np.flatnonzero(np.concatenate([[True], sid[1:] != sid[:-1]]))
    length = np.diff(np.concatenate([start, [n]]))
    live = sid[start] != 0
    start, length, owner = start[live], length[live], sid[start][live]
    acc = np.zeros((len(start), r.shape[1]), dtype)
    for j in range(int(length.max()) if len(length) else 0):
        sel = length > j
        acc[sel] = acc[sel] + r[order[start[sel] + j]]
        mag[owner[sel]] += np.abs(r[order[start[sel] + j]].astype(np.float64))
    out[owner] = out[owner] + acc
    run[owner] = length
    return out, mag, run
