"""The deterministic dense gradient (include/okge.h, okge_rows_to_dense) stated in NumPy.

The gradient of table row `id` is the sequential fp32 sum of its occurrence rows in ASCENDING occurrence position,
((g_a + g_b) + g_c) ...; a run's first row is taken as it is (not added to a zero: the sign of a zero survives).  With `into`, the
row the table already holds comes first: acc = into[id]; acc += g_a; acc += g_b; ...  Rows no occurrence names keep what `into`
holds (zero without one); ids outside [0, table_rows) are skipped."""
import numpy as np


def densify(ids, rows, table_rows, into=None):
    """ids (n,) integers, rows (n, row_len) float32 -> (table_rows, row_len) float32 (a new array; `into` is not modified)"""
    ids = np.asarray(ids).reshape(-1)
    rows = np.asarray(rows, dtype=np.float32)
    assert rows.ndim == 2 and rows.shape[0] == len(ids)                   # (n = 0: an (0, row_len) array)
    out = np.zeros((table_rows, rows.shape[1]), np.float32) if into is None else np.array(into, dtype=np.float32, copy=True)
    assert out.shape == (table_rows, rows.shape[1])
    started = np.zeros(table_rows, bool) if into is None else np.ones(table_rows, bool)
    for pos in range(len(ids)):                       # ascending position; one fp32 addition per occurrence row and column
        i = int(ids[pos])
        if i < 0 or i >= table_rows:
            continue
        if started[i]:
            out[i] = out[i] + rows[pos]               # (float32 + float32 -> float32: one rounding, no wider intermediate)
        else:
            out[i] = rows[pos]
            started[i] = True
    return out
