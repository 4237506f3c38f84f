"""tests/eval_loss_reference.py (the float64 statement the GPU tests hold the evaluators' validation loss to) against the
reference's own number for the whole FB15k-237 validation pass, and its two forms against each other.  CPU only."""
import numpy as np

import eval_loss_reference as ref
from conftest import golden
from oracle import kge_oracle as ko
from test_validation_pass import _producer, _tables


def pass_loss(z, tmp_path, dtype=np.float64):
    """sum of L and of B N over the 40 batches of the G13 pass, scores from the tables in `dtype`"""
    E, R = (a.astype(dtype) for a in _tables(z))
    C = E[2:]
    total, elems = 0.0, 0
    for cb in _producer(tmp_path, z, "cpu"):
        b = cb.batch
        parts = []
        if b.n_po:
            parts.append(ko.score_prefix(ko.COMPLEX, ko.DIR_PO, E[b.po_obj.numpy()], R[b.po_rel.numpy()], C))
        if b.n_sp:
            parts.append(ko.score_prefix(ko.COMPLEX, ko.DIR_SP, E[b.sp_subj.numpy()], R[b.sp_rel.numpy()], C))
        x = np.concatenate(parts)
        total += ref.eval_loss(x, cb.row_ptr.numpy(), cb.grp_ptr.numpy(), cb.ids.numpy(), "bce")
        elems += x.shape[0] * x.shape[1]
    return total, elems


def test_restatement_against_the_reference_pass(okge_lib, tmp_path):
    """sum L over the 40 G13 batches within 1e-4 relative of the reference's eval_loss_sum.  Measured: reference 478 087.613,
    float64 478 098.889, relative difference 2.36e-5 -- the reference's own fp32 reduction='sum' over 7.3 M elements per batch
    (an fp32 NumPy evaluation agrees with float64 to 1e-9); 1e-4 pins labels, sign and normaliser."""
    z = golden("g13_valid_pass_fb15k237")
    total, elems = pass_loss(z, tmp_path)
    want = float(z["eval_loss_sum"])
    print("reference", want, "float64", total, "relative", abs(total - want) / want)
    assert abs(total - want) <= 1e-4 * want
    assert elems == 292419510
    # the reference's average, quoted to six digits (+- 5e-9), under the same 1e-4
    assert abs(total / elems - 0.00163494) <= 1e-4 * 0.00163494 + 5e-9


def _random_case(rng, B, N, scale):
    x = rng.standard_normal((B, N)) * scale
    row_ptr, grp_ptr, ids = [0], [0], []
    for b in range(B):
        ng = 0 if b == 1 else int(rng.integers(1, 4))
        for g in range(ng):
            cols = rng.integers(0, N, int(rng.integers(1, 4))).tolist()
            if b == 2:
                cols = [5] + cols                 # every group of row 2 names column 5
            ids.extend(cols)
            grp_ptr.append(len(ids))
        row_ptr.append(len(grp_ptr) - 1)
    return x, np.asarray(row_ptr), np.asarray(grp_ptr), np.asarray(ids)


def test_decomposition_equals_elementwise():
    rng = np.random.default_rng(5)
    for B, N, scale in ((7, 40, 1.0), (5, 67, 30.0), (3, 300, 0.1)):
        x, row_ptr, grp_ptr, ids = _random_case(rng, B, N, scale)
        pos = ref.row_positives(row_ptr, grp_ptr, ids)
        assert len(pos[1]) == 0                                           # a row without groups
        g2 = [ids[grp_ptr[g]:grp_ptr[g + 1]] for g in range(row_ptr[2], row_ptr[3])]
        assert all(5 in g for g in g2) and (len(g2) < 2 or list(pos[2]).count(5) == 1)      # a repeated column counts once
        y = ref.labels(B, N, row_ptr, grp_ptr, ids)
        assert y.sum() == sum(len(p) for p in pos) and set(np.unique(y)) <= {0.0, 1.0}
        for eps in (0.0, 0.1):
            a, b = ref.bce_elementwise(x, y, eps), ref.bce_decomposed(x, pos, eps)
            assert abs(a - b) <= 1e-12 * abs(a), (eps, a, b)
        a, b = ref.kl_elementwise(x, y), ref.kl_decomposed(x, pos)
        assert abs(a - b) <= 1e-12 * abs(a), (a, b)
