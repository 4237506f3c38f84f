"""A plain numpy restatement of one token-pooling pass (okge_pool_encode_calls / okge_pool_backward_calls, csrc/okge_pool.hip)
at a chosen dtype -- float64 as the reference, float32 to calibrate error bounds.  Not a conftest: the tests import it (the
per-magnitude-band rule is lstm_reference.band_check).

One pass on ONE slot: the calls' rows one after the other (ids, or first_id .. first_id + n - 1) -> their token rows -> the
token table's rows, padded positions (token 0) included: row 0 is an ordinary row -> sum, mean (sum / (count(token > 0) + 1e-12))
or max over the positions -> `raw` -> per call BatchNorm1d (eps BN_EPS, momentum 0.1): training mode with the biased variance of
that call's own rows, the running mean and UNBIASED variance updated call after call, or eval mode with the running statistics
-> `out`.  Gradients are those of sum(out * d_out) with training-mode batch-norm: the batch-norm parameter gradients added up
in call order, the token-table gradient scattered in ascending (row, position) order; under max pooling a column's gradient
goes to the FIRST position that attains the column maximum; token 0 (padding_idx) never receives a gradient.  Every sum over
rows or positions is sequential in the chosen dtype (numpy reduces the leading axis row after row)."""
import numpy as np
import torch

from lstm_reference import row_ids

BN_MOMENTUM = 0.1


def pool_rows(W, t, pool):
    """W (vocab x d, the pass's dtype), t (rows x L token ids) -> (raw rows, lens or first-maximum positions)"""
    if pool == "max":
        emb = W[t]                                                     # (rows, L, d)
        arg = emb.argmax(axis=1)                                       # the first maximum
        return np.take_along_axis(emb, arg[:, None, :], axis=1)[:, 0, :], arg
    acc = np.zeros((t.shape[0], W.shape[1]), dtype=W.dtype)
    for j in range(t.shape[1]):
        acc += W[t[:, j]]
    lens = (t > 0).sum(1, keepdims=True).astype(W.dtype) + W.dtype.type(1e-12)
    return (acc / lens if pool == "mean" else acc), lens


def pool_pass(W, tok, calls, pool="sum", bn=None, running=None, training=True, d_out=None, dtype=torch.float64, order_seed=None):
    """W (vocab x d), tok (n_ids x max_len), calls [(ids or None, first_id, n)] on one slot, bn = (weight, bias) or None, running
    = (mean, var) or None (fresh: zeros, ones), d_out (rows x d) or None.  Returns a dict of float64 numpy arrays: raw, out
    (= raw without batch-norm); with batch-norm running_mean / running_var after the calls and, in training mode, saved_mean /
    saved_rstd (calls x d); with d_out dW and, with batch-norm, d_bn_weight / d_bn_bias.  order_seed: scatter the token-table
    gradient in a seeded random order of the pairs instead of the ascending one (what float atomics may do)."""
    from open_knowledge_graph_embeddings_amd.token_pooled import BN_EPS
    dt = np.float64 if dtype in (torch.float64, np.float64) else np.float32
    as_np = lambda x: (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(dt)      # noqa: E731
    Wd = as_np(W)
    d = Wd.shape[1]
    t = tok.detach().cpu()[row_ids(calls)].numpy().astype(np.int64)
    raw, extra = pool_rows(Wd, t, pool)
    res, out = {"raw": raw}, raw
    xhat, rstd, means = [], [], []
    if bn is not None:
        w, b = as_np(bn[0]), as_np(bn[1])
        rm, rv = (np.zeros(d, dt), np.ones(d, dt)) if running is None else (as_np(running[0]).copy(), as_np(running[1]).copy())
        eps, mom = dt(BN_EPS), dt(BN_MOMENTUM)
        out, r0 = np.empty_like(raw), 0
        for _, _, n in calls:
            x = raw[r0:r0 + n]
            if training:
                mean = x.sum(0) / dt(n)
                var = ((x - mean) ** 2).sum(0) / dt(n)
                rs = dt(1) / np.sqrt(var + eps)
                xhat.append((x - mean) * rs)
                rstd.append(rs)
                out[r0:r0 + n] = xhat[-1] * w + b
                rm += mom * (mean - rm)
                rv += mom * (var * dt(n) / dt(max(n - 1, 1)) - rv)
                means.append(mean)
            else:
                out[r0:r0 + n] = (x - rm) / np.sqrt(rv + eps) * w + b
            r0 += n
        res["running_mean"], res["running_var"] = rm, rv
        if training:
            res["saved_mean"], res["saved_rstd"] = np.stack(means), np.stack(rstd)
    res["out"] = out
    if d_out is not None:
        assert bn is None or training, "the backward is that of training-mode batch-norm"
        dx = as_np(d_out).copy()
        if bn is not None:
            dw_, db_, r0 = np.zeros(d, dt), np.zeros(d, dt), 0
            for c, (_, _, n) in enumerate(calls):
                dy = dx[r0:r0 + n].copy()
                dbias, dweight = dy.sum(0), (dy * xhat[c]).sum(0)
                dx[r0:r0 + n] = w * rstd[c] * (dy - dbias / dt(n) - xhat[c] * dweight / dt(n))
                db_ += dbias
                dw_ += dweight
                r0 += n
            res["d_bn_weight"], res["d_bn_bias"] = dw_, db_
        dW = np.zeros_like(Wd)
        if pool == "max":
            winner = np.take_along_axis(t, extra, axis=1)              # (rows, d): the token each column's gradient goes to
            cols = np.broadcast_to(np.arange(d), winner.shape)
            sel = winner != 0
            rows_, cols_, g_ = winner[sel], cols[sel], dx[sel]         # row-major: ascending row, then column
            if order_seed is not None:
                perm = np.random.default_rng(order_seed).permutation(rows_.size)
                rows_, cols_, g_ = rows_[perm], cols_[perm], g_[perm]
            np.add.at(dW, (rows_, cols_), g_)
        else:
            if pool == "mean":
                dx = dx / extra
            flat = t.reshape(-1)
            pairs = np.nonzero(flat != 0)[0]                          # ascending (row, position)
            if order_seed is not None:
                pairs = np.random.default_rng(order_seed).permutation(pairs)
            np.add.at(dW, flat[pairs], dx[pairs // t.shape[1]])
        res["dW"] = dW
    return {k: np.asarray(v, dtype=np.float64) for k, v in res.items()}
