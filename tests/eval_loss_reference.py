"""The validation loss of an evaluation batch in float64 NumPy: what Trainer.compute_one_batch(training=False) reports
(openkge/trainer.py:93-106, :263-271; labels: openkge/dataset.py:864-935) on eval-mode, UNFILTERED scores x (B, N).

Labels: y[b][n] = 1 for every candidate column named by any answer group of row b -- the union of the row's ids in the
row_ptr / grp_ptr / ids CSR, as a set (a column named by two groups counts once).
BCE, smoothing eps:  y' = (y + 1/N)(1 - eps) if eps > 0 else y;  L = sum max(x,0) - x y' + log1p(e^-|x|)
KL:                  unnormalised labels, no smoothing;  L = KLDiv(sum)(log_softmax(x), y) = -sum_{y = 1} log_softmax(x)
Meter: loss.update(L / (B N), B N) per batch, so a pass averages sum L / sum B N with count sum B N.

Two statements of each: elementwise over the (B, N) block, and the per-row decomposition the kernels use
    BCE  sum_b S_b - (1 - eps)(P_b + X_b / N)   (eps = 0: S_b - P_b),  S_b = sum_n softplus(x), X_b = sum_n x, P_b = sum_{pos} x
    KL   sum_b npos_b lse_b - P_b"""
import numpy as np


def row_positives(row_ptr, grp_ptr, ids):
    """per row, the sorted distinct candidate columns its answer groups name"""
    row_ptr, grp_ptr, ids = (np.asarray(a) for a in (row_ptr, grp_ptr, ids))
    return [np.unique(ids[grp_ptr[row_ptr[b]]:grp_ptr[row_ptr[b + 1]]]).astype(np.int64) for b in range(len(row_ptr) - 1)]


def labels(B, N, row_ptr, grp_ptr, ids):
    y = np.zeros((B, N), np.float64)
    for b, cols in enumerate(row_positives(row_ptr, grp_ptr, ids)):
        y[b, cols] = 1.0
    return y


def softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def bce_elementwise(x, y, eps=0.0):
    x = np.asarray(x, np.float64)
    if eps > 0:
        y = (y + 1.0 / x.shape[1]) * (1.0 - eps)
    return float((softplus(x) - x * y).sum())


def row_lse(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def kl_elementwise(x, y):
    x = np.asarray(x, np.float64)
    return float(-(y * (x - row_lse(x)[:, None])).sum())


def bce_decomposed(x, pos, eps=0.0):
    x = np.asarray(x, np.float64)
    N = x.shape[1]
    S, X = softplus(x).sum(axis=1), x.sum(axis=1)
    P = np.array([x[b, cols].sum() for b, cols in enumerate(pos)])
    return float((S - (1.0 - eps) * (P + X / N)).sum() if eps > 0 else (S - P).sum())


def kl_decomposed(x, pos):
    x = np.asarray(x, np.float64)
    lse = row_lse(x)
    return float(sum(len(cols) * lse[b] - x[b, cols].sum() for b, cols in enumerate(pos) if len(cols)))


def kl_scale(x, pos):
    """what a KL loss is held against: L is a difference of sum npos |lse| and sum |x_pos|"""
    x = np.asarray(x, np.float64)
    lse = row_lse(x)
    return float(sum(len(cols) * abs(lse[b]) + np.abs(x[b, cols]).sum() for b, cols in enumerate(pos)))


def eval_loss(x, row_ptr, grp_ptr, ids, loss="bce", eps=0.0):
    """L of one batch from its score block and answer-group CSR (the decomposed form)"""
    pos = row_positives(row_ptr, grp_ptr, ids)
    assert len(pos) == np.shape(x)[0]
    return bce_decomposed(x, pos, eps) if loss == "bce" else kl_decomposed(x, pos)
