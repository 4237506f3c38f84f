"""Top-k link prediction: which entities does the model predict for (s, p, ?) / (?, p, o).

What a caller of the reference reads off ``sp_prefix_score`` / ``po_prefix_score`` (openkge/model.py:52-74) with ``torch.topk``
under the evaluation's filter (openkge/dataset.py:423-453), without the (B, N) score block: ``okge_topk_prefixes`` sweeps the
candidates in ranges, keeps per 64-candidate tile and row the tile's best k records and folds them into the (B, k) result.
The order (include/okge.h, "top-k link prediction"): higher score first, equal scores by the smaller candidate column, NaN as
-inf, filtered columns excluded, short rows padded with (-inf, -1, -1).  ``sharded.ShardedTopKPredictor`` is the same over an
entity table sharded across ranks.
"""
from __future__ import annotations

from . import _native as N
from . import hotpath as H


def batch_and_filter(batch, filt_ptr=None, filt_col=None):
    """a PrefixBatch, or a dataset.CollatedBatch (built with is_training_data=False: its filter CSR is used unless one is
    passed) -> (PrefixBatch, filt_ptr, filt_col)"""
    if not isinstance(batch, H.PrefixBatch):
        cb = batch
        batch = cb.batch
        if filt_ptr is None and filt_col is None:
            filt_ptr, filt_col = cb.filt_ptr, cb.filt_col
    return batch, filt_ptr, filt_col


class TopKPredictor:
    """Single device.  run() -> (scores (B, k) fp32, ids (B, k) int32 entity ids, cols (B, k) int32 candidate columns)."""

    def __init__(self, E, R, scorer, k, engine=None, range_n=None):
        N.refuse_bias_scorer(scorer, type(self).__name__)
        self.E, self.R, self.scorer, self.k = E, R, scorer, int(k)
        self.range_n = 0 if range_n is None else int(range_n)
        self.engine = engine or H.HotPath(E.device)

    def run(self, batch, filt_ptr=None, filt_col=None):
        batch, filt_ptr, filt_col = batch_and_filter(batch, filt_ptr, filt_col)
        scores, cols, ids = self.engine.topk_prefixes(self.E, self.R, self.scorer, batch, self.k, filt_ptr, filt_col, self.range_n)
        return scores, ids, cols
